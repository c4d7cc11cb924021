// extern "C" test hooks of librsys_hip.so that take no handle (declared in include/rsys_debug.h): raw device memory, one launcher per
// call on caller-provided device buffers, the GEMM route.  Every op hook runs its launchers on the null stream and synchronises.
#include <algorithm>
#include <string.h>

#include "model_internal.hpp"

using namespace rsys;

namespace {
// Device scratch of one hook call: every buffer a hook allocates comes from here and is freed, behind a device synchronise, on every
// return path.  Declared before a HookDet of the same call, so that the order of the two is fixed.
struct HookScratch {
  const char* who;
  std::vector<void*> bufs;
  explicit HookScratch(const char* who_) : who(who_) {}
  ~HookScratch() { hipDeviceSynchronize(); for (void* p : bufs) hipFree(p); }
  int alloc(void** p, size_t bytes) {
    if (hipMalloc(p, bytes ? bytes : 16) != hipSuccess) {
      (void)hipGetLastError();
      *p = nullptr;
      set_error(std::string(who) + ": no device memory for the call's scratch");
      return RSYS_ERR_HIP;
    }
    bufs.push_back(*p);
    return RSYS_OK;
  }
  template <typename T> int get(T** p, size_t count) { return alloc((void**)p, count * sizeof(T)); }
};
// The end of every hook, on the status of its launches: always synchronises; a failed launch's code comes back with the launch's
// message untouched, otherwise the synchronise's status.
int hook_finish(int rc) {
  if (rc) { (void)hipDeviceSynchronize(); return rc; }
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}
// Deterministic-mode scratch of one hook call: installed in g_det for that call only (as DetScope does for a model), its two buffers
// taken from the call's HookScratch.  check() fails unless the launch took the partial-sum branch with no launch falling back to
// atomics for want of scratch.
struct HookDet {
  DetScratch saved;
  bool on;
  explicit HookDet(bool on_) : saved(g_det), on(on_) { g_det = DetScratch(); }
  ~HookDet() { hipDeviceSynchronize(); g_det = saved; }
  // part_floats for the launch's partial rows; the two-stage reduction needs ceil(partial rows / 32) * row length floats
  int alloc(HookScratch& scratch, long long part_floats, long long tmp_floats) {
    if (!on) return RSYS_OK;
    part_floats = std::max(part_floats, 1LL); tmp_floats = std::max(tmp_floats, 1LL);
    float *part = nullptr, *tmp = nullptr;
    RC(scratch.get(&part, (size_t)part_floats));
    RC(scratch.get(&tmp, (size_t)tmp_floats));
    g_det.part = part; g_det.cap = part_floats; g_det.tmp = tmp; g_det.tmp_cap = tmp_floats;
    return RSYS_OK;
  }
  int check(const char* who) {
    if (!on) return RSYS_OK;
    if (g_det.part_used < 1 || g_det.part_short != 0) {
      set_error(std::string(who) + ": the deterministic partial-sum branch did not run");
      return RSYS_ERR_STATE;
    }
    return RSYS_OK;
  }
};
long long ceil32(long long n) { return (n + 31) / 32; }
// a launch of a launcher with an ordered branch: in deterministic mode it must have counted itself in g_det.part_used
struct DetTook {
  const HookDet& det; int before;
  explicit DetTook(const HookDet& d) : det(d), before(g_det.part_used) {}
  int check(const char* who) const {
    if (!det.on || (g_det.part_used > before && g_det.part_short == 0)) return RSYS_OK;
    set_error(std::string(who) + ": the ordered (deterministic) branch did not run");
    return RSYS_ERR_STATE;
  }
};
// an index array that addresses a caller buffer, copied back for the host checks
int hook_ints(const int32_t* dev, long long n, std::vector<int>& out) {
  out.resize((size_t)std::max(n, 0LL));
  if (n > 0) HIP_CHECK(hipMemcpy(out.data(), dev, (size_t)n * 4, hipMemcpyDeviceToHost));
  return RSYS_OK;
}
// The tile maps of one attention hook call, as every one of them builds them before its first attention launch: a map set from the
// call's scratch, applied to p, one launch_attn_tilemap on the null stream.  rsys_op_attention_maps alone passes the rest: fill = every
// byte of the set holds 0xA5 before the first launch (an entry the kernels leave unwritten then shows), uid_prev / tm_prev = an
// earlier launch on those tokens into the same set (a model reuses one set step after step).
int hook_attn_maps(HookScratch& scratch, AttnParams& p, AttnMaps& maps, bool fill = false, const int32_t* uid_prev = nullptr,
                   const int32_t* tm_prev = nullptr) {
  RC(attn_maps_alloc(maps, p.B, p.T, p.H, p.KV, [&](void** b, size_t bytes) { return scratch.alloc(b, bytes); }));
  maps.apply(p);
  if (fill) {
    const size_t nt = (size_t)(p.T + 63) / 64;
    HIP_CHECK(hipMemsetAsync(maps.zero_base, 0xA5, 12 * maps.map_bytes, nullptr));
    HIP_CHECK(hipMemsetAsync(maps.order_q, 0xA5, (size_t)p.B * p.H * nt * 4, nullptr));
    HIP_CHECK(hipMemsetAsync(maps.order_k, 0xA5, (size_t)p.B * p.KV * nt * 4, nullptr));
    HIP_CHECK(hipMemsetAsync(maps.qbits, 0xA5, (size_t)p.B * nt * nt * 64 * 8, nullptr));
    HIP_CHECK(hipMemsetAsync(maps.kbits, 0xA5, (size_t)p.B * nt * nt * 64 * 8, nullptr));
  }
  if (uid_prev != nullptr) {
    AttnParams prev = p;
    prev.uid = uid_prev; prev.tm = tm_prev;
    RC(launch_attn_tilemap(prev, nullptr));
  }
  return launch_attn_tilemap(p, nullptr);
}
// one product of the split-K weight-gradient forms as grouped_weight_grads / f8_dw_params build it
GemmParams hook_dw_params(const void* A, const void* B, void* C, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc,
                          int32_t f8, const float* f8_desc, int32_t f8_rseg, int32_t f8_rowmode) {
  GemmParams p{};
  p.A = A; p.B = B; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.c_f32 = 1; p.epi = EPI_ATOMIC; p.alpha = 1.f; p.splitk = 1;
  p.f8 = f8; p.f8_desc = f8_desc; p.f8_rseg = f8_rseg; p.f8_rowmode = f8_rowmode;
  return p;
}
// expr, which names the element type Elt, with Elt = bf16 for RSYS_DTYPE_BF16 and Elt = float for any other dtype (a hook that takes
// only the two checks its dtype first)
#define BY_DTYPE(dtype, ...) \
  ((dtype) == RSYS_DTYPE_BF16 ? [&] { using Elt = bf16; return (__VA_ARGS__); }() : [&] { using Elt = float; return (__VA_ARGS__); }())
}  // namespace

extern "C" {

// ---------------------------------------------------------------- raw device helpers + per-op entry points (tests)
int32_t rsys_dev_alloc(void** p, size_t bytes) { HIP_CHECK(hipMalloc(p, bytes ? bytes : 16)); HIP_CHECK(hipMemset(*p, 0, bytes ? bytes : 16)); return RSYS_OK; }
int32_t rsys_dev_free(void* p) { HIP_CHECK(hipFree(p)); return RSYS_OK; }
int32_t rsys_dev_h2d(void* d, const void* s, size_t n) { HIP_CHECK(hipMemcpy(d, s, n, hipMemcpyHostToDevice)); return RSYS_OK; }
int32_t rsys_dev_d2h(void* d, const void* s, size_t n) { HIP_CHECK(hipDeviceSynchronize()); HIP_CHECK(hipMemcpy(d, s, n, hipMemcpyDeviceToHost)); return RSYS_OK; }
int32_t rsys_dev_memset(void* d, int v, size_t n) { HIP_CHECK(hipMemset(d, v, n)); return RSYS_OK; }

int32_t rsys_op_gemm(int32_t dtype, const void* A, const void* B, void* C, int32_t M, int32_t N, int32_t K, int64_t lda,
                     int64_t ldb, int64_t ldc, int32_t a_km, int32_t b_km, int32_t a_f32, int32_t c_f32, int32_t splitk) {
  switches_parse();
  GemmParams p{};
  p.A = A; p.B = B; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.c_f32 = c_f32; p.splitk = splitk < 1 ? 1 : splitk; p.alpha = 1.f;
  p.epi = p.splitk > 1 ? EPI_ATOMIC : EPI_STORE;
  if (sw().debug_epi >= 0) p.epi = sw().debug_epi;   // timing experiments only (e.g. 99 = no epilogue)
  // (written out: a_f32 is the bf16 arm's alone)
  return hook_finish(dtype == RSYS_DTYPE_BF16 ? launch_gemm<bf16>(p, a_f32 != 0, false, a_km != 0, b_km != 0, nullptr)
                                              : launch_gemm<float>(p, false, false, a_km != 0, b_km != 0, nullptr));
}

int32_t rsys_op_gemm_rows(int32_t dtype, const void* A, const void* B, void* C, int32_t M, int32_t N, int32_t K, int64_t lda,
                          int64_t ldb, int64_t ldc, int32_t b_km, int32_t c_f32, const int32_t* rows_dev) {
  switches_parse();
  ARG_CHECK(rows_dev != nullptr, "rsys_op_gemm_rows: rows_dev is null");
  GemmParams p{};
  p.A = A; p.B = B; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.c_f32 = c_f32 != 0; p.splitk = 1; p.alpha = 1.f; p.epi = EPI_STORE; p.m_dev = rows_dev;
  if (c_f32 == 3) { p.epi = EPI_ATOMIC; p.splitk = 8; }   // the head's dEw form: fp32 C accumulated by split-K atomics
  return hook_finish(BY_DTYPE(dtype, launch_gemm<Elt>(p, false, false, false, b_km != 0, nullptr)));
}

int32_t rsys_op_gemm_klimit(int32_t dtype, const void* A, const void* B, void* C, int32_t M, int32_t N, int32_t K, int64_t lda,
                            int64_t ldb, int64_t ldc, int32_t accumulate, const int32_t* k_dev) {
  switches_parse();
  ARG_CHECK(k_dev != nullptr, "rsys_op_gemm_klimit: k_dev is null");
  GemmParams p{};
  p.A = A; p.B = B; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.c_f32 = 1; p.splitk = 1; p.alpha = 1.f; p.epi = accumulate ? EPI_ACCUM : EPI_STORE; p.k_dev = k_dev;
  return hook_finish(BY_DTYPE(dtype, launch_gemm<Elt>(p, false, false, true, true, nullptr)));
}

int32_t rsys_op_gemm_epi(int32_t dtype, const void* A, const void* B, void* C, int32_t M, int32_t N, int32_t K, int64_t lda,
                         int64_t ldb, int64_t ldc, int32_t b_km, int32_t c_f32, int32_t epi, float alpha, int32_t accum,
                         const float* bias, const float* resid, int64_t ldr, void* C2, int64_t ldc2, const float* E,
                         const float* rope_cos, const float* rope_sin, const float* rope_cs, const int32_t* rope_pos, int32_t T,
                         int32_t hd, int32_t n_q, int32_t n_k, const int32_t* m_dev, char* tag, int32_t tag_bytes, int32_t* half) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_gemm_epi: dtype is fp32 or bf16");
  ARG_CHECK(A != nullptr && B != nullptr && C != nullptr, "rsys_op_gemm_epi: null operand");
  ARG_CHECK(tag != nullptr && tag_bytes >= 4 && half != nullptr, "rsys_op_gemm_epi: null output");
  ARG_CHECK(epi >= EPI_STORE && epi <= EPI_SWIGLU_BWD && epi != EPI_ATOMIC, "rsys_op_gemm_epi: epilogue is one of GemmEpi without EPI_ATOMIC");
  // the operands an epilogue dereferences (the launchers take them on trust)
  if (epi == EPI_BIAS || epi == EPI_TABLE || epi == EPI_GELU) ARG_CHECK(bias != nullptr, "rsys_op_gemm_epi: this epilogue reads bias");
  if (epi == EPI_RESIDUAL) ARG_CHECK(resid != nullptr, "rsys_op_gemm_epi: EPI_RESIDUAL reads resid");
  if (epi == EPI_TABLE) ARG_CHECK(E != nullptr, "rsys_op_gemm_epi: EPI_TABLE reads E");
  if (epi == EPI_SWIGLU || epi == EPI_TABLE || epi == EPI_GELU || epi == EPI_SWIGLU_BWD) ARG_CHECK(C2 != nullptr, "rsys_op_gemm_epi: this epilogue needs C2");
  if (epi == EPI_QKV_ROPE) ARG_CHECK(rope_cos != nullptr && rope_sin != nullptr, "rsys_op_gemm_epi: EPI_QKV_ROPE reads rope_cos / rope_sin");
  GemmParams p{};
  p.A = A; p.B = B; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.c_f32 = c_f32 != 0; p.splitk = 1; p.epi = epi; p.alpha = alpha; p.accum = accum != 0;
  p.bias = bias; p.resid = resid; p.ldr = ldr; p.C2 = C2; p.ldc2 = ldc2; p.E = E;
  p.rope_cos = rope_cos; p.rope_sin = rope_sin; p.rope_cs = rope_cs; p.rope_pos = rope_pos; p.T = T; p.hd = hd; p.n_q = n_q; p.n_k = n_k;
  p.m_dev = m_dev;
  RC(hook_finish(BY_DTYPE(dtype, launch_gemm<Elt>(p, false, false, false, b_km != 0, nullptr))));
  // what launch_gemm just decided, from the same parameters and switches
  const GemmRoute r = BY_DTYPE(dtype, gemm_route<Elt>(p, false, false, false, b_km != 0, cu_count()));
  snprintf(tag, tag_bytes, "%s", gemm_kernel_tags[r.kernel]);
  *half = r.kernel == GK_8C && gemm8c_uses_half(p, cu_count()) ? 1 : 0;
  return RSYS_OK;
}

// the routing of launch_gemm, on the host only: a GemmParams from the fields the route reads (pointer fields only as set / unset)
int32_t rsys_debug_gemm_route(int32_t dtype, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc, int32_t a_km,
                              int32_t b_km, int32_t a_f32, int32_t c_f32, int32_t epi, int32_t splitk, int32_t flags, float alpha,
                              int32_t accum, int32_t set, int32_t m_expect, int32_t cus, char* tag, int32_t tag_bytes, int32_t* splits) {
  ARG_CHECK(tag != nullptr && tag_bytes >= 4 && splits != nullptr, "rsys_debug_gemm_route: null output");
  static int dummy[4];   // (never dereferenced: the route only tests these for null)
  GemmParams p{};
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc; p.ldc2 = ldc; p.ldr = ldc;
  p.c_f32 = c_f32; p.epi = epi; p.splitk = splitk; p.flags = flags; p.alpha = alpha; p.accum = accum; p.m_expect = m_expect;
  if (set & 1) p.m_dev = dummy;
  if (set & 2) p.k_dev = dummy;
  if (set & 4) p.slab = (float*)dummy;
  if (set & 8) p.rope_cs = (const float*)dummy;
  if (set & 16) p.rope_pos = dummy;
  if (set & 32) p.C2 = dummy;
  const GemmRoute r = dtype == RSYS_DTYPE_BF16 ? gemm_route<bf16>(p, a_f32 != 0, false, a_km != 0, b_km != 0, cus)
                                                : gemm_route<float>(p, false, false, a_km != 0, b_km != 0, cus);
  snprintf(tag, tag_bytes, "%s", gemm_kernel_tags[r.kernel]);
  *splits = r.splitk;
  return RSYS_OK;
}

// the check and the packer of an upload (model_batch.hip), on the host only: the caller's limits and buffer in place of a model's
int32_t rsys_debug_batch_pack(const rsys_batch* b, const int32_t limits[9], int32_t row_len, void* stage, int64_t stage_bytes,
                              int64_t offsets[30], int64_t* total_bytes, int32_t* distinct_ids) {
  ARG_CHECK(limits && stage && offsets && total_bytes && distinct_ids, "rsys_debug_batch_pack: null argument");
  const BatchLimits lim{limits[0], limits[1], limits[2], limits[3], limits[4], limits[5], limits[6], limits[7], limits[8]};
  std::vector<unsigned long long> id_seen;
  int distinct = 0;
  RC(batch_check(lim, b, row_len, &id_seen, &distinct));
  const BlobLayout L = blob_layout((size_t)b->rows * row_len);
  if ((int64_t)L.bytes > stage_bytes) { set_error("rsys_debug_batch_pack: staging buffer too small"); return RSYS_ERR_STATE; }
  batch_pack(lim, b, row_len, L, (unsigned char*)stage);
  int n = 0;
  for (size_t at : {L.time, L.userid, L.tmid, L.gender, L.source, L.matchedid, L.status, L.rating, L.progress}) offsets[n++] = (int64_t)at;
  for (int k = 0; k < 6; ++k) { offsets[n++] = (int64_t)L.label[k]; offsets[n++] = (int64_t)L.weight[k]; offsets[n++] = (int64_t)L.position[k]; }
  offsets[n++] = (int64_t)L.wm; offsets[n++] = (int64_t)L.rm; offsets[n++] = (int64_t)L.rope;
  *total_bytes = (int64_t)L.bytes; *distinct_ids = distinct;
  return RSYS_OK;
}

int32_t rsys_op_f8_quantize(const void* src, int64_t ld_src, int32_t rows, int32_t cols, int32_t fmt, int32_t layout, int32_t seg_cols,
                            int32_t seg_rep, void* dst, int64_t ld_dst, float* amax_dev, float* desc_dev, const float* wamax_dev,
                            int32_t n_w, int32_t w_rep, int32_t desc_mode) {
  switches_parse();
  ARG_CHECK(src && dst && amax_dev, "rsys_op_f8_quantize: null buffer");
  F8Cast c{};
  c.src = src; c.ld_src = ld_src; c.rows = rows; c.cols = cols; c.fmt = fmt; c.layout = layout; c.seg_cols = seg_cols; c.seg_rep = seg_rep < 1 ? 1 : seg_rep;
  c.amax = amax_dev; c.dst = (unsigned char*)dst; c.ld_dst = ld_dst; c.desc = desc_dev; c.wamax = wamax_dev; c.n_w = n_w; c.w_rep = w_rep < 1 ? 1 : w_rep;
  c.desc_mode = desc_mode;
  HIP_CHECK(hipMemsetAsync(amax_dev, 0, (size_t)F8_AMAX_SHARDS * F8_AMAX_SHARD * 4, nullptr));
  int rc = launch_f8_amax(c, nullptr);
  if (!rc) rc = launch_f8_cast(c, nullptr);
  return hook_finish(rc);
}

int32_t rsys_op_f8_weights(const float* src, int64_t ld, int32_t rows, int32_t cols, int32_t layout, int32_t seg_rows, int32_t seg_rep,
                           float* amax_dev, void* dst, void* dst_t, int64_t ld_t) {
  switches_parse();
  ARG_CHECK(src && dst && amax_dev, "rsys_op_f8_weights: null buffer");
  ARG_CHECK(cols % 4 == 0 && rows % 16 == 0, "rsys_op_f8_weights: rows % 16, cols % 4");
  F8WeightJob j{};
  j.src = src; j.ld = ld; j.rows = rows; j.cols = cols; j.layout = layout; j.seg_rows = seg_rows; j.seg_rep = seg_rep < 1 ? 1 : seg_rep; j.amax = amax_dev;
  j.dst = (unsigned char*)dst; j.dst_t = (unsigned char*)dst_t; j.ld_t = ld_t;
  const int ntiles = ((rows + 63) / 64) * ((cols + 63) / 64);
  std::vector<int> tj(ntiles, 0); int first = 0;
  HookScratch scratch("rsys_op_f8_weights");
  void* dev = nullptr;
  RC(scratch.alloc(&dev, sizeof(F8WeightJob) + 256 + (size_t)ntiles * 4 + 64));
  F8WeightJob* dj = (F8WeightJob*)dev; int* dfirst = (int*)((char*)dev + ((sizeof(F8WeightJob) + 63) / 64) * 64); int* dtj = dfirst + 16;
  bool ok = hipMemcpy(dj, &j, sizeof(j), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dfirst, &first, 4, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dtj, tj.data(), (size_t)ntiles * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemset(amax_dev, 0, 16) == hipSuccess;
  if (!ok) { set_error("rsys_op_f8_weights: job upload failed"); return RSYS_ERR_HIP; }
  return hook_finish(launch_f8_weights(dj, dtj, dfirst, ntiles, nullptr));
}

int32_t rsys_op_gemm_f8(const void* A8, const void* B8, void* C, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc,
                        int32_t a_fmt, int32_t c_f32, const float* desc_dev, int32_t seg_cols, int32_t alt, int32_t kb0, int32_t kb1,
                        int32_t kb2) {
  switches_parse();
  GemmParams p{};
  p.A = A8; p.B = B8; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.c_f32 = c_f32; p.splitk = 1; p.alpha = 1.f; p.epi = EPI_STORE;
  p.f8 = a_fmt == F8_E5M2 ? 2 : 1; p.f8_desc = desc_dev; p.f8_seg_cols = seg_cols; p.f8_alt = alt; p.f8_kb[0] = kb0; p.f8_kb[1] = kb1; p.f8_kb[2] = kb2;
  return hook_finish(launch_gemm8p_f8(p, nullptr));
}

int32_t rsys_op_gemm_group(int32_t n, const void* const* A, const void* const* B, void* const* C, const int32_t* M, const int32_t* N,
                           const int32_t* K, const int64_t* lda, const int64_t* ldb, const int64_t* ldc, const int32_t* f8,
                           const float* const* f8_desc, const int32_t* f8_rseg, const int32_t* f8_rowmode, int32_t ordered,
                           int32_t launches, int32_t* splitk_out, int32_t* kernel_out) {
  switches_parse();
  ARG_CHECK(n >= 0 && n <= 4096, "rsys_op_gemm_group: n outside 0..4096 (the plan takes 1..128 and says so)");
  ARG_CHECK(n == 0 || (A && B && C && M && N && K && lda && ldb && ldc && f8 && f8_desc && f8_rseg && f8_rowmode), "rsys_op_gemm_group: null array");
  ARG_CHECK(launches >= 1 && splitk_out != nullptr && kernel_out != nullptr, "rsys_op_gemm_group: launches >= 1, outputs not null");
  std::vector<GemmParams> ps((size_t)n);
  for (int i = 0; i < n; ++i) {
    ARG_CHECK(A[i] != nullptr && B[i] != nullptr && C[i] != nullptr, "rsys_op_gemm_group: null operand");
    ps[i] = hook_dw_params(A[i], B[i], C[i], M[i], N[i], K[i], lda[i], ldb[i], ldc[i], f8[i], f8_desc[i], f8_rseg[i], f8_rowmode[i]);
  }
  GemmGroupPlan* pl = nullptr;
  RC(gemm8p_group_plan_create(ps.data(), n, &pl, ordered != 0));
  *splitk_out = gemm8p_group_splitk(pl);
  *kernel_out = ps[0].f8 != 0 ? RSYS_GROUP_KERNEL_8GF : (gemm8p_group_on_4k(pl) ? RSYS_GROUP_KERNEL_4KG : RSYS_GROUP_KERNEL_8G);
  int rc = RSYS_OK;
  for (int i = 0; i < launches && rc == RSYS_OK; ++i) rc = launch_gemm8p_group(pl, nullptr);
  rc = hook_finish(rc);
  gemm8p_group_plan_destroy(pl);   // (behind the synchronise: the plan owns the work lists and the slabs)
  return rc;
}

int32_t rsys_op_gemm_f8_splitk(const void* A8, const void* B8, void* C, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc,
                               const float* desc_dev, int32_t rseg, int32_t rowmode, int32_t launches) {
  switches_parse();
  ARG_CHECK(A8 != nullptr && B8 != nullptr && C != nullptr, "rsys_op_gemm_f8_splitk: null operand");
  ARG_CHECK(launches >= 1, "rsys_op_gemm_f8_splitk: launches >= 1");
  const GemmParams p = hook_dw_params(A8, B8, C, M, N, K, lda, ldb, ldc, 2, desc_dev, rseg, rowmode);
  int rc = RSYS_OK;
  for (int i = 0; i < launches && rc == RSYS_OK; ++i) rc = launch_gemm8p_f8_splitk(p, nullptr);
  return hook_finish(rc);
}

int32_t rsys_op_attention(int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv,
                          const int32_t* uid, const int32_t* tm, void* O, float* lse, const void* dO, void* dqkv,
                          const float* rope_cos, const float* rope_sin) {
  return rsys_op_attention_ex(dtype, B, T, H, KV, hd, qkv, uid, tm, O, lse, dO, dqkv, rope_cos, rope_sin, nullptr, T, nullptr, nullptr, nullptr);
}

int32_t rsys_op_attention_ex(int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv,
                             const int32_t* uid, const int32_t* tm, void* O, float* lse, const void* dO, void* dqkv,
                             const float* rope_cos, const float* rope_sin, const int32_t* rope_pos, int32_t rope_rows,
                             const int32_t* q_active, float* amax_fwd, float* amax_bwd) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_attention: dtype fp32 or bf16");
  ARG_CHECK(B >= 1 && T >= 1 && H >= 1 && KV >= 1 && qkv && uid && tm && O && lse, "rsys_op_attention: null or empty");
  ARG_CHECK(!dO || (dqkv && rope_cos && rope_sin), "rsys_op_attention: the backward needs dqkv and the rope tables");
  if (dO && rope_pos) {   // every explicit position inside the tables (one copy back)
    std::vector<int32_t> pos((size_t)B * T);
    HIP_CHECK(hipMemcpy(pos.data(), rope_pos, pos.size() * 4, hipMemcpyDeviceToHost));
    for (int32_t v : pos) ARG_CHECK(v >= 0 && v < rope_rows, "rsys_op_attention: rope_pos outside the tables");
  } else if (dO) {
    ARG_CHECK(rope_rows >= T, "rsys_op_attention: rope tables shorter than T");
  }
  const size_t e = dtype == RSYS_DTYPE_BF16 ? 2 : 4;
  AttnParams p{};
  p.B = B; p.T = T; p.H = H; p.KV = KV; p.hd = hd; p.is_bf16 = dtype == RSYS_DTYPE_BF16;
  p.q = qkv; p.k = (const unsigned char*)qkv + (size_t)H * hd * e; p.v = (const unsigned char*)qkv + (size_t)(H + KV) * hd * e;
  p.ld = (long long)(H + 2 * KV) * hd;
  p.o = O; p.ldo = (long long)H * hd; p.lse = lse; p.uid = uid; p.tm = tm;
  HookScratch scratch("rsys_op_attention");
  AttnMaps maps; float* delta = nullptr;
  RC(scratch.get(&delta, (size_t)B * H * T));
  p.delta = delta;
  p.dO = dO; p.dq = dqkv; p.dk = (unsigned char*)dqkv + (size_t)H * hd * e;
  p.dv = (unsigned char*)dqkv + (size_t)(H + KV) * hd * e; p.ldg = p.ld;
  p.rope_cos = rope_cos; p.rope_sin = rope_sin; p.rope_pos = rope_pos; p.q_active = q_active;
  // (delta of the query tiles beyond q_active is never written: NaN there, so that a dK/dV kernel that reads it shows)
  if (q_active) HIP_CHECK(hipMemsetAsync(delta, 0xFF, sizeof(float) * B * H * T, nullptr));
  int rc = hook_attn_maps(scratch, p, maps);
  p.f8_amax = amax_fwd;
  if (!rc) rc = BY_DTYPE(dtype, launch_attn_fwd<Elt>(p, nullptr));
  p.f8_amax = amax_bwd;
  if (!rc && dO) rc = BY_DTYPE(dtype, launch_attn_bwd<Elt>(p, nullptr));
  return hook_finish(rc);
}

// attn_sel_kernel alone: the tile maps are built here, as rsys_op_attention_ex builds them; sel is checked on the host
int32_t rsys_op_attention_selected(int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv, const int32_t* uid,
                                   const int32_t* tm, int32_t n_sel, const int32_t* sel, void* O) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_attention_selected: dtype fp32 or bf16");
  ARG_CHECK(B >= 1 && T >= 1 && H >= 1 && KV >= 1 && n_sel >= 1 && qkv && uid && tm && sel && O, "rsys_op_attention_selected: null or empty");
  ARG_CHECK((long long)B * T < (1ll << 31), "rsys_op_attention_selected: B * T must stay below 2^31");
  {
    std::vector<int32_t> hs((size_t)n_sel);
    HIP_CHECK(hipMemcpy(hs.data(), sel, hs.size() * 4, hipMemcpyDeviceToHost));
    for (int32_t v : hs) ARG_CHECK(v >= 0 && v < B * T, "rsys_op_attention_selected: a selected token outside [0, B * T)");
  }
  const size_t e = dtype == RSYS_DTYPE_BF16 ? 2 : 4;
  AttnParams p{};
  p.B = B; p.T = T; p.H = H; p.KV = KV; p.hd = hd; p.is_bf16 = dtype == RSYS_DTYPE_BF16;
  p.q = qkv; p.k = (const unsigned char*)qkv + (size_t)H * hd * e; p.v = (const unsigned char*)qkv + (size_t)(H + KV) * hd * e;
  p.ld = (long long)(H + 2 * KV) * hd; p.uid = uid; p.tm = tm;
  HookScratch scratch("rsys_op_attention_selected");
  AttnMaps maps;
  int rc = hook_attn_maps(scratch, p, maps);
  if (!rc) rc = BY_DTYPE(dtype, launch_attn_sel<Elt>(p, sel, n_sel, O, (long long)H * hd, nullptr));
  return hook_finish(rc);
}

// launch_attn_tilemap alone, through hook_attn_maps as the two hooks above reach it; no attention kernel runs
int32_t rsys_op_attention_maps(int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t KV, int32_t hd, const int32_t* uid, const int32_t* tm,
                               const int32_t* q_active, const int32_t* uid_prev, const int32_t* tm_prev, void* qmap, void* kmap,
                               void* qmap_full, void* kmap_full, void* qmap16, void* kmap16, uint64_t* qbits, uint64_t* kbits,
                               int32_t* order_q, int32_t* order_k, int32_t* info) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_attention_maps: dtype fp32 or bf16");
  ARG_CHECK(B >= 1 && T >= 1 && H >= 1 && KV >= 1 && hd >= 1 && uid && tm, "rsys_op_attention_maps: null or empty");
  ARG_CHECK(H % KV == 0, "rsys_op_attention_maps: H must be a multiple of KV");
  ARG_CHECK(T % 8 == 0 && T <= 4096, "rsys_op_attention_maps: T must be a multiple of 8 and <= 4096");
  ARG_CHECK((uid_prev == nullptr) == (tm_prev == nullptr), "rsys_op_attention_maps: uid_prev and tm_prev come together");
  ARG_CHECK(qmap && kmap && qmap_full && kmap_full && qmap16 && kmap16 && qbits && kbits && order_q && order_k && info,
            "rsys_op_attention_maps: null output");
  const size_t nt = (size_t)(T + 63) / 64, n_tok = (size_t)B * T;
  {   // the token keys' ranges (attn_tilemap_kernel takes them on trust) and q_active, one copy back each
    std::vector<int> h;
    for (const int32_t* ids : {uid, uid_prev}) {
      if (ids == nullptr) continue;
      RC(hook_ints(ids, (long long)n_tok, h));
      for (int v : h) ARG_CHECK(v >= 0 && v < (1 << 19), "rsys_op_attention_maps: a uid outside [0, 2^19)");
    }
    for (const int32_t* ids : {tm, tm_prev}) {
      if (ids == nullptr) continue;
      RC(hook_ints(ids, (long long)n_tok, h));
      for (int v : h) ARG_CHECK(v >= 0 && v < 4096, "rsys_op_attention_maps: a tm outside [0, 4096)");
    }
    if (q_active != nullptr) {
      RC(hook_ints(q_active, B, h));
      for (int v : h) ARG_CHECK(v >= 0 && v <= (int)nt, "rsys_op_attention_maps: q_active outside [0, ceil(T / 64)]");
    }
  }
  AttnParams p{};
  p.B = B; p.T = T; p.H = H; p.KV = KV; p.hd = hd; p.is_bf16 = dtype == RSYS_DTYPE_BF16;
  p.uid = uid; p.tm = tm; p.q_active = q_active;
  HookScratch scratch("rsys_op_attention_maps");
  AttnMaps maps;
  RC(hook_finish(hook_attn_maps(scratch, p, maps, true, uid_prev, tm_prev)));
  const size_t mapb = (size_t)B * nt * 4 * attn_map_words(T), bitb = (size_t)B * nt * nt * 64 * 8;
  HIP_CHECK(hipMemcpy(qmap, maps.qmap, mapb, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(kmap, maps.kmap, mapb, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(qmap_full, maps.qmap_full, mapb, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(kmap_full, maps.kmap_full, mapb, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(qmap16, maps.qmap16, 4 * mapb, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(kmap16, maps.kmap16, 4 * mapb, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(qbits, maps.qbits, bitb, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(kbits, maps.kbits, bitb, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(order_q, maps.order_q, (size_t)B * H * nt * 4, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(order_k, maps.order_k, (size_t)B * KV * nt * 4, hipMemcpyDeviceToHost));
  const AttnOrderPlan o = attn_order_plan(p);
  const int32_t facts[8] = {attn_map_words(T), o.R, o.kv_pairs, o.lists == 8 ? 1 : 0, o.n_inner_q, o.n_inner_k, o.identity, (int32_t)nt};
  memcpy(info, facts, sizeof(facts));
  return RSYS_OK;
}

int32_t rsys_op_attention_cached(int32_t dtype, int32_t rows, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv, const void* cache,
                                 int32_t n_slots, const int32_t* slot, const int32_t* n_hist, const int32_t* n_cand, void* O) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "dtype: fp32 or bf16");
  ARG_CHECK(qkv && cache && slot && n_hist && n_cand && O && KV >= 1 && H >= 1, "null or empty");
  CandAttnParams p{};
  p.rows = rows; p.T = T; p.H = H; p.KV = KV; p.hd = hd;
  p.qkv = qkv; p.ld = (long long)(H + 2 * KV) * hd; p.cache = cache; p.n_slots = n_slots;
  p.slot = slot; p.n_hist = n_hist; p.n_cand = n_cand; p.o = O; p.ldo = (long long)H * hd;
  return hook_finish(BY_DTYPE(dtype, launch_attn_cand<Elt>(p, nullptr)));
}

// attn_cand_tiles_kernel alone: the host's segments (row, first_tile, n_cand, slot, n_hist) are checked (inside their rows, no tile twice, slots
// and counts in range) and become the kernel's two device tables for the length of the call
int32_t rsys_op_attention_cached_tiles(int32_t dtype, int32_t rows, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv, const void* cache,
                                       int32_t n_slots, int32_t Tc, int32_t n_seg, const int32_t* seg, void* O) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "dtype: fp32 or bf16");
  ARG_CHECK(qkv && cache && seg && O && KV >= 1 && H >= 1 && rows >= 1 && T >= 8 && n_slots >= 1, "null or empty");
  if (Tc == 0) Tc = T;
  TileOwners tiles(rows, T / 2);   // (a row of T tokens holds T / 2 interaction columns; ceil(T / 64) tiles)
  ARG_CHECK(n_seg >= 1 && n_seg <= rows * tiles.nt, "1 <= n_seg <= rows x ceil(T / 64)");
  std::vector<int> tab((size_t)4 * n_seg, -1);
  for (int i = 0; i < n_seg; ++i) {
    const int r = seg[5 * i], ft = seg[5 * i + 1], nc = seg[5 * i + 2], sl = seg[5 * i + 3], nh = seg[5 * i + 4];
    ARG_CHECK(ft >= 0 && ft < tiles.nt && nc >= 1, "segment outside its row");
    ARG_CHECK(sl >= 0 && sl < n_slots && nh >= 0 && 2 * nh <= Tc, "segment's slot or n_hist out of range");
    RC(tiles.place("rsys_op_attention_cached_tiles", r, 32 * ft, nc, i));
    tab[4 * i] = sl; tab[4 * i + 1] = nh; tab[4 * i + 2] = ft; tab[4 * i + 3] = nc;
  }
  tab.insert(tab.end(), tiles.owner.begin(), tiles.owner.end());
  HookScratch scratch("rsys_op_attention_cached_tiles");   // (after the segment checks: they return with nothing allocated)
  int* d_tab = nullptr;
  RC(scratch.get(&d_tab, tab.size()));
  HIP_CHECK(hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  CandAttnParams p{};
  p.rows = rows; p.T = T; p.Tc = Tc; p.H = H; p.KV = KV; p.hd = hd;
  p.qkv = qkv; p.ld = (long long)(H + 2 * KV) * hd; p.cache = cache; p.n_slots = n_slots;
  p.seg = d_tab; p.tile_seg = d_tab + 4 * n_seg; p.n_seg = n_seg; p.o = O; p.ldo = (long long)H * hd;
  return hook_finish(BY_DTYPE(dtype, launch_attn_cand<Elt>(p, nullptr)));
}

// rank_cache_copy_segments_kernel alone: the host's descriptors (row, first column, n_hist, slot) are checked against the rows and the cache
int32_t rsys_op_rank_cache_copy_segments(int32_t dtype, int32_t rows, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv, void* cache,
                                         int32_t n_slots, int32_t Tc, int32_t n_seg, const int32_t* seg) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "dtype: fp32 or bf16");
  ARG_CHECK(qkv && cache && seg && KV >= 1 && H >= 1 && hd >= 1 && rows >= 1 && T >= 2 && n_slots >= 1 && n_seg >= 1 && n_seg <= 65535, "null or empty");
  if (Tc == 0) Tc = T;
  for (int i = 0; i < n_seg; ++i) {
    const int r = seg[4 * i], c0 = seg[4 * i + 1], nh = seg[4 * i + 2], sl = seg[4 * i + 3];
    ARG_CHECK(r >= 0 && r < rows && c0 >= 0 && nh >= 0 && 2 * ((long long)c0 + nh) <= T && 2 * (long long)nh <= Tc, "segment outside its row or longer than a slot");
    ARG_CHECK(sl >= 0 && sl < n_slots, "slot outside the cache");
  }
  HookScratch scratch("rsys_op_rank_cache_copy_segments");   // (after the segment checks: they return with nothing allocated)
  int* d_seg = nullptr;
  RC(scratch.get(&d_seg, (size_t)4 * n_seg));
  HIP_CHECK(hipMemcpy(d_seg, seg, (size_t)4 * n_seg * 4, hipMemcpyHostToDevice));
  const long long ld = (long long)(H + 2 * KV) * hd;
  return hook_finish(BY_DTYPE(dtype, launch_rank_cache_copy_segments<Elt>((const Elt*)qkv, ld, H * hd, 2 * KV * hd, T, Tc, rows, d_seg, n_seg, n_slots,
                                                                           (Elt*)cache, nullptr)));
}

int32_t rsys_op_topk(const float* scores, int64_t ld, int32_t rows, int32_t V, int32_t k, int32_t* ids, float* vals, int32_t* counts) {
  switches_parse();
  return op_topk(scores, ld, rows, V, k, ids, vals, counts);
}
int32_t rsys_op_topk_window(const float* scores, int64_t ld, int32_t rows, int32_t V, const int64_t* start, const int32_t* len,
                            int32_t* ids, float* vals, int32_t* counts, int32_t* totals, int32_t* bounds) {
  switches_parse();
  return op_topk_window(scores, ld, rows, V, start, len, ids, vals, counts, totals, bounds);
}
int32_t rsys_op_lse(const float* z, int64_t ldz, int32_t rows, int32_t V, float* lse) {
  switches_parse();
  return op_lse(z, ldz, rows, V, lse);
}
int32_t rsys_op_query_weights(const float* z, int64_t ldz, const float* lse, const int32_t* members, const int32_t* ranges, int32_t q0,
                              const float* user_w, int32_t n_groups, const float* src, float* dst, int32_t V, int32_t last,
                              const int64_t* cand_offsets, const int32_t* cand, const float* r_masked, const int64_t* rm_offsets,
                              const float* retrieval_coef, const float* rating_coefs, float rating_mean, int32_t first, float* sc,
                              const int64_t* sel_offsets, const int32_t* sel_medium, const int32_t* sel_ids, int32_t medium, const float* emb_m,
                              const float* X, int32_t dim, const float* sel_w, float* S) {
  switches_parse();
  ARG_CHECK(dst || sc || S, "rsys_op_query_weights: no section asked for (dst, sc and S are all NULL)");
  if (dst) RC(op_combine_weighted(src, dst, n_groups, V, last, z, ldz, lse, members, ranges, q0, user_w));
  if (sc) RC(op_rank_score_weighted(n_groups, cand_offsets, cand, z, ldz, lse, members, ranges, q0, r_masked, rm_offsets, retrieval_coef,
                                    rating_coefs, rating_mean, first, user_w, sc));
  if (S) RC(op_selected_sum_weighted(n_groups, sel_offsets, sel_medium, sel_ids, medium, emb_m, X, dim, sel_w, S));
  return RSYS_OK;
}
int32_t rsys_op_target_rank(const float* scores, int64_t ld, int32_t rows, int32_t V, const int32_t* targets, int32_t* rank_out) {
  switches_parse();
  return op_target_rank(scores, ld, rows, V, targets, rank_out);
}
int32_t rsys_op_pair_ranks(const float* scores, int64_t ld, int32_t rows, int32_t V, const int32_t* self, const int64_t* tgt_offsets,
                           const int32_t* tgt_ids, int32_t* ranks_out) {
  switches_parse();
  return op_pair_ranks(scores, ld, rows, V, self, tgt_offsets, tgt_ids, ranks_out);
}
int32_t rsys_op_rerank(int32_t n, int32_t partialk, const float* pen, const float* r, const float* gram, const int32_t* ss_bits,
                       const int32_t* related_bits, int32_t* picks) {
  switches_parse();
  return op_rerank(n, partialk, pen, r, gram, ss_bits, related_bits, picks);
}
// the backward's embedding scatter on caller-provided device buffers: gE[id'] += sum_n gx0[n * ldx ..+D) over the tokens whose
// masked id (m_matchedid, -1 -> row V) is id'; the token index is built from the raw ids (matchedid) as at batch upload.
// atomic != 0 runs the float-atomic form instead (A/B reference).
int32_t rsys_op_embedding_scatter(const float* gx0, int64_t ldx, const int32_t* matchedid, const int32_t* m_matchedid, int32_t N,
                                  int32_t V, int32_t D, float* gE, int32_t atomic) {
  switches_parse();
  ARG_CHECK(gx0 && matchedid && m_matchedid && gE && N >= 1 && ldx >= D, "rsys_op_embedding_scatter: arguments");
  if (atomic) {
    ARG_CHECK(ldx == 2LL * D, "the atomic form reads the interleaved layout (row stride 2 D)");
    BatchDev b{}; b.N = N; b.m_matchedid = const_cast<int*>(m_matchedid);
    return hook_finish(launch_embedding_scatter_add(gx0, b, V, D, gE, nullptr));
  }
  HookScratch scratch("rsys_op_embedding_scatter");
  unsigned long long* keys = nullptr; int *skey = nullptr, *sidx = nullptr; float* slab = nullptr;
  RC(scratch.get(&keys, (size_t)token_index_capacity(N)));
  RC(scratch.get(&skey, (size_t)N));
  RC(scratch.get(&sidx, (size_t)N));
  RC(scratch.get(&slab, (size_t)seg_scatter_slab_floats(N, D)));
  int rc = launch_token_index_build(matchedid, N, V, keys, skey, sidx, nullptr);
  if (!rc) rc = launch_embedding_scatter_segmented(gx0, ldx, m_matchedid, skey, sidx, N, V, D, gE, slab, nullptr);
  return hook_finish(rc);
}

// ---------------------------------------------------------------- row kernels and the optimiser on caller-provided buffers (tests)
int32_t rsys_op_rmsnorm_fwd(int32_t dtype, const float* x, const float* scale, void* y, float* rstd, int64_t rows, int32_t D,
                            const int32_t* rows_dev, const int32_t* in_rows, float* amax) {
  switches_parse();
  ARG_CHECK(x && scale && y && rows >= 1, "rsys_op_rmsnorm_fwd: arguments");
  return hook_finish(BY_DTYPE(dtype, launch_rmsnorm_fwd<Elt>(x, scale, (Elt*)y, rstd, rows, D, nullptr, rows_dev, in_rows, amax)));
}

int32_t rsys_op_rmsnorm_bwd(int32_t dtype, int32_t g_f32, const void* g, const float* x, const float* scale, const float* rstd,
                            const float* resid, const int32_t* resid_slot, const int32_t* io_rows, const int32_t* rows_dev,
                            float* dx, void* dx_t, float* dscale, int64_t rows, int32_t D, float* amax, int32_t deterministic) {
  switches_parse();
  ARG_CHECK(g && x && scale && rstd && dx && dscale && rows >= 0, "rsys_op_rmsnorm_bwd: arguments");
  ARG_CHECK(!g_f32 || (resid_slot == nullptr && io_rows == nullptr), "rsys_op_rmsnorm_bwd: the f32-gradient form takes no resid_slot / io_rows");
  HookScratch scratch("rsys_op_rmsnorm_bwd");
  HookDet det(deterministic != 0);
  const long long wgs = std::max<long long>(1, std::min<long long>(rows, 4LL * std::max(1, sw().debug_norm_bwd_grid)));   // >= the launch's grid
  RC(det.alloc(scratch, wgs * D, ceil32(wgs) * D));
  int rc;
  if (g_f32) rc = BY_DTYPE(dtype, launch_rmsnorm_bwd_f32<Elt>((const float*)g, x, scale, rstd, resid, dx, (Elt*)dx_t, dscale, rows, D, nullptr, rows_dev, amax));
  else rc = BY_DTYPE(dtype, launch_rmsnorm_bwd<Elt>((const Elt*)g, x, scale, rstd, resid, dx, (Elt*)dx_t, dscale, rows, D, nullptr, rows_dev, resid_slot, io_rows, amax));
  RC(hook_finish(rc));
  return det.check("rsys_op_rmsnorm_bwd");
}

int32_t rsys_op_ce(int32_t dtype, void* logits, int64_t ldl, int32_t n, int32_t V, const int32_t* idx, const float* label,
                   const float* weight, const int32_t* position, const float* stats, const int32_t* npos, float task_w, float* loss,
                   int32_t deterministic) {
  switches_parse();
  ARG_CHECK(logits && idx && label && weight && position && stats && loss && n >= 0 && V >= 1, "rsys_op_ce: arguments");
  HookScratch scratch("rsys_op_ce");
  HookDet det(deterministic != 0 && n > 0);
  RC(det.alloc(scratch, n, ceil32(n)));
  RC(hook_finish(BY_DTYPE(dtype, launch_ce_fwd_bwd<Elt>((Elt*)logits, ldl, n, V, idx, label, weight, position, stats, npos, task_w, loss, nullptr))));
  return det.check("rsys_op_ce");
}

int32_t rsys_op_rating_tail(int32_t dtype, void* z, const void* hact, int32_t n, int32_t D, const float* w2, const float* b2,
                            const int32_t* idx, const float* label, const float* weight, const float* stats, float rating_mean,
                            float task_w, int32_t evaluate, float* loss, float* dw2, float* db2, float* db0, const int32_t* npos,
                            int32_t deterministic) {
  switches_parse();
  ARG_CHECK(z && hact && w2 && b2 && idx && label && weight && stats && loss && dw2 && db2 && db0 && n >= 0, "rsys_op_rating_tail: arguments");
  HookScratch scratch("rsys_op_rating_tail");
  HookDet det(deterministic != 0 && n > 0);
  const long long grid = std::min<long long>((n + 3) / 4, 512);   // the launcher's grid
  RC(det.alloc(scratch, grid * (2LL * D + 4), ceil32(grid) * D));
  RC(hook_finish(BY_DTYPE(dtype, launch_rating_tail<Elt>((Elt*)z, (const Elt*)hact, n, D, w2, b2, idx, label, weight, stats, rating_mean, task_w, evaluate,
                                                         loss, dw2, db2, db0, nullptr, npos))));
  return det.check("rsys_op_rating_tail");
}

int32_t rsys_op_sumsq(const float* g, int64_t n, float* out) {
  ARG_CHECK(g && out, "rsys_op_sumsq: arguments");
  HookScratch scratch("rsys_op_sumsq");
  float* part = nullptr;
  RC(scratch.get(&part, (size_t)sumsq_parts()));
  return hook_finish(launch_sumsq(g, n, out, part, nullptr, true));
}

int32_t rsys_op_clip_adamw(int32_t dtype, float* p, float* g, float* m, float* v, void* shadow, int64_t n_decay, int64_t n_total,
                           float lr, float b1, float b2, float eps, float wd, int32_t step, float max_norm, float grad_div,
                           int32_t zero_grad, int64_t sh_skip_lo, int64_t sh_skip_hi, int32_t fused, float* sumsq) {
  switches_parse();
  ARG_CHECK(p && g && m && v && sumsq && n_total >= 4 && step >= 1, "rsys_op_clip_adamw: arguments");
  HookScratch scratch("rsys_op_clip_adamw");
  float* part = nullptr;
  RC(scratch.get(&part, (size_t)sumsq_parts()));
  const bool bf = dtype == RSYS_DTYPE_BF16;   // (the two arms stay written out: the shadow arguments are the bf16 arm's alone)
  int rc = launch_sumsq(g, n_total, sumsq, part, nullptr, true);
  if (fused) {   // optimizer_step: the clip coefficient and the 1 / grad_div inside AdamW
    const float* ss = max_norm > 0.f ? sumsq : nullptr;
    if (!rc) rc = bf ? launch_adamw<bf16>(p, g, m, v, (bf16*)shadow, n_decay, n_total, lr, b1, b2, eps, wd, step, ss, grad_div, max_norm, zero_grad, nullptr,
                                          sh_skip_lo, sh_skip_hi)
                     : launch_adamw<float>(p, g, m, v, nullptr, n_decay, n_total, lr, b1, b2, eps, wd, step, ss, grad_div, max_norm, zero_grad, nullptr);
  } else {       // clip_grad_norm_ (model_clip: a scale pass over the gradients), then AdamW with no clip
    if (!rc) rc = launch_scale(g, n_total, sumsq, grad_div, max_norm, nullptr);
    if (!rc) rc = bf ? launch_adamw<bf16>(p, g, m, v, (bf16*)shadow, n_decay, n_total, lr, b1, b2, eps, wd, step, nullptr, 1.f, 0.f, zero_grad, nullptr,
                                          sh_skip_lo, sh_skip_hi)
                     : launch_adamw<float>(p, g, m, v, nullptr, n_decay, n_total, lr, b1, b2, eps, wd, step, nullptr, 1.f, 0.f, zero_grad, nullptr);
  }
  return hook_finish(rc);
}

// the adapter bank's kernels on caller-provided buffers (adapter_bank.hip: the launch routines the model path calls)
int32_t rsys_op_adapter_bank(int32_t dtype, int32_t stages, int32_t train, int32_t rows, int32_t Ttok, int32_t D, int32_t H, int32_t KV, int32_t hd,
                             int32_t L, int32_t layer, float p, uint64_t seed, int64_t stream, const int32_t* row_slot, const void* bankA,
                             const void* bankB, const void* xn, void* La, void* qkv, const void* dqkv, void* dLa, void* dxn, float* partA, float* partB,
                             float* gA, float* gB, const float* rope_cos, const float* rope_sin, const int32_t* rope_pos, int32_t rope_rows) {
  switches_parse();
  return adapter_bank_op(dtype, stages, train, rows, Ttok, D, H, KV, hd, L, layer, p, seed, stream, row_slot, bankA, bankB, xn, La, qkv, dqkv, dLa, dxn,
                         partA, partB, gA, gB, rope_cos, rope_sin, rope_pos, rope_rows);
}

int32_t rsys_op_adapter_bank_tiles(int32_t dtype, int32_t stages, int32_t rows, int32_t Ttok, int32_t D, int32_t H, int32_t KV, int32_t hd, int32_t L,
                                   int32_t layer, const int32_t* tile_slot, const void* bankA, const void* bankB, const void* xn, void* La, void* qkv,
                                   const float* rope_cos, const float* rope_sin, const int32_t* rope_pos, int32_t rope_rows) {
  switches_parse();
  return adapter_bank_op(dtype, stages, 0, rows, Ttok, D, H, KV, hd, L, layer, 0.f, 0, 0, tile_slot, bankA, bankB, xn, La, qkv, nullptr, nullptr, nullptr,
                         nullptr, nullptr, nullptr, nullptr, rope_cos, rope_sin, rope_pos, rope_rows, 1);
}

int32_t rsys_op_adapter_bank_segments(int32_t dtype, int32_t stages, int32_t train, int32_t rows, int32_t Ttok, int32_t D, int32_t H, int32_t KV, int32_t hd,
                                      int32_t L, int32_t layer, float p, uint64_t seed, int64_t stream, const int32_t* segs, int32_t n_seg, const void* bankA,
                                      const void* bankB, const void* xn, void* La, void* qkv, const void* dqkv, void* dLa, void* dxn, float* partA,
                                      float* partB, float* gA, float* gB, const float* rope_cos, const float* rope_sin, const int32_t* rope_pos,
                                      int32_t rope_rows) {
  switches_parse();
  return adapter_bank_op(dtype, stages, train, rows, Ttok, D, H, KV, hd, L, layer, p, seed, stream, segs, bankA, bankB, xn, La, qkv, dqkv, dLa, dxn, partA,
                         partB, gA, gB, rope_cos, rope_sin, rope_pos, rope_rows, 2, n_seg);
}

int32_t rsys_op_adapter_bank_adamw(int32_t dtype, float* A32, float* B32, float* gA, float* gB, float* mA, float* vA, float* mB, float* vB, void* A,
                                   void* B, int64_t nA, int64_t nB, const float* per_slot, float b1, float b2, float eps, float wd, float* norms) {
  switches_parse();
  return adapter_bank_adamw_op(dtype, A32, B32, gA, gB, mA, vA, mB, vB, A, B, nA, nB, per_slot, b1, b2, eps, wd, norms);
}

int32_t rsys_op_dropout(int32_t dtype, const void* src, void* dst, int64_t n, float p, uint64_t seed, int64_t stream, int32_t accumulate) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_dropout: dtype fp32 or bf16");
  ARG_CHECK(src && dst && n >= 1 && p >= 0.f && p < 1.f && stream >= 0 && stream <= 0xFFFFFFFFLL, "rsys_op_dropout: arguments");
  return hook_finish(BY_DTYPE(dtype, launch_dropout<Elt>((const Elt*)src, (Elt*)dst, n, p, seed, (unsigned int)stream, accumulate, nullptr)));
}

// ---------------------------------------------------------------- the sharded-table kernels on caller-provided buffers (shard.hip)
// Each stage calls the launch routine the model path calls, unchanged, on the null stream.  No collective and no GEMM: the caller stands
// in for both.  Index arrays that address caller buffers are copied back once (hook_ints) and checked before anything is launched.

int32_t rsys_op_vp_ce(int32_t dtype, int32_t stages, int32_t deterministic, const int32_t* idx, const float* label, const float* weight,
                      const int32_t* position, const float* stats, const int32_t* npos, float task_w, int32_t KB, int32_t KBmax, float* own,
                      const void* EwAll, const float* metaAll, int32_t W, int32_t D, void* EwC, float* metaC, int32_t* nlive, int32_t* pre,
                      void* logits, int64_t ldl, int32_t Vloc, int32_t col0, float* lmax, const float* gmax, float* sums, int32_t cap,
                      int32_t rank, float* loss, int32_t rows, int32_t rows_finish) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_vp_ce: dtype fp32 or bf16");
  ARG_CHECK(stages > 0 && stages < 32, "rsys_op_vp_ce: stages is a mask of 1, 2, 4, 8, 16");
  const bool bf = dtype == RSYS_DTYPE_BF16;
  const int E = bf ? 8 : 4;
  if (stages & 1) ARG_CHECK(idx && label && weight && position && stats && npos && own && KB >= 0 && KB <= KBmax && KBmax >= 1, "rsys_op_vp_ce: meta arguments");
  if (stages & 2) ARG_CHECK(EwAll && metaAll && EwC && metaC && nlive && pre && W >= 1 && W <= 47 && KBmax >= 1 && D >= E && D % E == 0, "rsys_op_vp_ce: compact arguments");
  if (stages & (4 | 16)) ARG_CHECK(cap >= 1 && metaC && nlive && sums && Vloc >= 0 && ldl >= 0 && ldl % 8 == 0 && Vloc <= ldl, "rsys_op_vp_ce: cap >= 1, Vloc <= ldl, ldl a multiple of 8");
  if (stages & 4) ARG_CHECK(lmax && rows >= 0 && rows <= cap && (Vloc == 0 || logits), "rsys_op_vp_ce: stats arguments (rows <= cap)");
  if (stages & 8) ARG_CHECK(lmax && gmax && sums && rows >= 0, "rsys_op_vp_ce: rebase arguments");
  if (stages & 16) ARG_CHECK(gmax && pre && loss && rank >= 0 && rank < 47 && rows_finish >= 0 && rows_finish <= cap && (ldl == 0 || logits), "rsys_op_vp_ce: finish arguments (rows_finish <= cap)");
  HookScratch scratch("rsys_op_vp_ce");
  HookDet det(deterministic != 0 && (stages & 16) && rows_finish > 0);
  RC(det.alloc(scratch, rows_finish, ceil32(rows_finish)));
  const auto run = [&]() -> int {
    if (stages & 1) RC(launch_vp_meta(idx, label, weight, position, stats, npos, task_w, KB, KBmax, own, nullptr));
    if (stages & 2) RC(BY_DTYPE(dtype, launch_vp_compact<Elt>((const Elt*)EwAll, metaAll, W, KBmax, D, (Elt*)EwC, metaC, nlive, pre, nullptr)));
    if ((stages & 4) && rows > 0) RC(BY_DTYPE(dtype, launch_vp_stats<Elt>((const Elt*)logits, ldl, Vloc, col0, metaC, nlive, lmax, sums, cap, rows, nullptr)));
    if ((stages & 8) && rows > 0) RC(launch_vp_rebase(lmax, gmax, sums, rows, nullptr));
    if ((stages & 16) && rows_finish > 0) {
      DetTook took(det);
      RC(BY_DTYPE(dtype, launch_vp_finish<Elt>((Elt*)logits, ldl, Vloc, col0, metaC, gmax, sums, cap, nlive, pre, rank, loss, rows_finish, nullptr)));
      RC(took.check("rsys_op_vp_ce"));
    }
    return RSYS_OK;
  };
  return hook_finish(run());
}

int32_t rsys_op_ss(int32_t dtype, int32_t stages, int32_t deterministic, int32_t len, int32_t n_s, int32_t n_tot, int32_t col0, uint64_t seed,
                   int64_t stream, int32_t* cols, int32_t* bitmap, int32_t* tlist, int32_t* tcount, const float* metaC, const int32_t* nlive,
                   const int32_t* pre, int32_t rank, int32_t cap_rows, int32_t rows, int32_t rows_finish, const void* EwC, const void* Floc,
                   int32_t D, void* logits, int64_t ldl, float* lmax, float* lsum, float* tl, float* gmax, float* loss, float* dt,
                   float* gE_loc, float* dEwC, const int32_t* ridx, int32_t rbase, int64_t rld, int32_t rn, int32_t rtable_rows,
                   const void* gsrc, void* gdst, const float* asrc, float* adst) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_ss: dtype fp32 or bf16");
  ARG_CHECK(stages > 0 && stages < 2048, "rsys_op_ss: stages is a mask of 1 .. 1024");
  const bool bf = dtype == RSYS_DTYPE_BF16;
  const int E = bf ? 8 : 4;
  ARG_CHECK(len >= 0 && n_s >= 0 && n_tot >= n_s, "rsys_op_ss: len >= 0, 0 <= n_s <= n_tot");
  if (stages & 1) ARG_CHECK(cols && stream >= 0 && stream <= 0xFFFFFFFFLL, "rsys_op_ss: sample arguments");
  if (stages & 2) ARG_CHECK(metaC && nlive && bitmap && tlist && tcount && cap_rows >= 1 && len >= 1, "rsys_op_ss: targets arguments");
  if (stages & 4) ARG_CHECK(cols && bitmap && n_s >= 1, "rsys_op_ss: drop_hits arguments");
  if (stages & (8 | 512)) ARG_CHECK(ridx && rn >= 1 && rtable_rows >= 1 && D >= 4 && rld >= D, "rsys_op_ss: plain row copy arguments");
  if (stages & 8) ARG_CHECK(gsrc && gdst && D % E == 0 && rld % E == 0, "rsys_op_ss: gather_rows_plain arguments");
  if (stages & 512) ARG_CHECK(asrc && adst && D % 4 == 0 && rld % 4 == 0, "rsys_op_ss: add_rows_plain arguments");
  if (stages & (16 | 32 | 64 | 128 | 256 | 1024)) ARG_CHECK(rows >= 0, "rsys_op_ss: rows");
  if (stages & (16 | 1024)) ARG_CHECK(EwC && Floc && metaC && nlive && D >= 1 && len >= 1, "rsys_op_ss: target row arguments");
  if (stages & 16) ARG_CHECK(tl, "rsys_op_ss: target_logit arguments");
  if (stages & (32 | 256)) ARG_CHECK(metaC && nlive && (n_tot == 0 || (logits && cols)) && ldl >= n_tot && len >= n_s, "rsys_op_ss: logits arguments (ldl >= n_tot)");
  if (stages & 32) ARG_CHECK(lmax && lsum, "rsys_op_ss: stats arguments");
  if (stages & 64) ARG_CHECK(lmax && tl && gmax, "rsys_op_ss: max_with_target arguments");
  if (stages & 128) ARG_CHECK(lmax && gmax && lsum, "rsys_op_ss: rebase arguments");
  if (stages & 256) ARG_CHECK(logits && ldl >= 1 && gmax && lsum && tl && pre && loss && dt && rank >= 0 && rank < 47 && rows_finish >= 0, "rsys_op_ss: finish arguments");
  if (stages & 1024) ARG_CHECK(dt && gE_loc && dEwC, "rsys_op_ss: target_grad arguments");
  std::vector<int> h;
  if ((stages & 4) && !(stages & 1)) {   // drop_hits reads the bitmap at cols[j]
    RC(hook_ints(cols, n_s, h));
    for (int c : h) ARG_CHECK(c >= 0 && c < len, "rsys_op_ss: drop_hits takes columns in [0, len)");
  }
  if (stages & (8 | 512)) {
    RC(hook_ints(ridx, rn, h));
    for (int c : h) ARG_CHECK(c < 0 || ((long long)rbase + c >= 0 && (long long)rbase + c < rtable_rows), "rsys_op_ss: a row index outside the table");
  }
  const bool det_stage = ((stages & 256) && rows_finish > 0) || ((stages & 1024) && rows > 0);
  HookScratch scratch("rsys_op_ss");
  HookDet det(deterministic != 0 && det_stage);
  RC(det.alloc(scratch, rows_finish, ceil32(rows_finish)));
  const unsigned int st = (unsigned int)stream;
  const auto run = [&]() -> int {
    if (stages & 1) RC(launch_ss_sample(len, n_s, seed, st, cols, nullptr));
    if (stages & 2) RC(launch_ss_targets(metaC, nlive, cap_rows, len, col0, (unsigned int*)bitmap, tlist, tcount, nullptr));
    if (stages & 4) RC(launch_ss_drop_hits(cols, n_s, (const unsigned int*)bitmap, nullptr));
    if (stages & 8) RC(BY_DTYPE(dtype, launch_gather_rows_plain<Elt>((const Elt*)gsrc, rld, ridx, rbase, (Elt*)gdst, rn, D, nullptr)));
    if ((stages & 16) && rows > 0)
      RC(BY_DTYPE(dtype, launch_ss_target_logit<Elt>((const Elt*)EwC, (const Elt*)Floc, D, len, col0, metaC, nlive, tl, rows, nullptr)));
    if ((stages & 32) && rows > 0)
      RC(BY_DTYPE(dtype, launch_ss_stats<Elt>((const Elt*)logits, ldl, n_s, n_tot, len, col0, cols, metaC, nlive, lmax, lsum, rows, nullptr)));
    if ((stages & 64) && rows > 0) RC(launch_ss_max_with_target(lmax, tl, gmax, rows, nullptr));
    if ((stages & 128) && rows > 0) RC(launch_ss_rebase(lmax, gmax, lsum, rows, nullptr));
    if ((stages & 256) && rows_finish > 0) {
      DetTook took(det);
      RC(BY_DTYPE(dtype, launch_ss_finish<Elt>((Elt*)logits, ldl, n_s, n_tot, len, col0, cols, metaC, gmax, lsum, tl, nlive, pre, rank, loss, dt, rows_finish,
                                               nullptr)));
      RC(took.check("rsys_op_ss (finish)"));
    }
    if (stages & 512) RC(launch_add_rows_plain(asrc, ridx, rbase, adst, rld, rn, D, nullptr));
    if ((stages & 1024) && rows > 0) {
      DetTook took(det);
      RC(BY_DTYPE(dtype, launch_ss_target_grad<Elt>((const Elt*)EwC, (const Elt*)Floc, D, len, col0, metaC, dt, nlive, gE_loc, dEwC, rows, nullptr)));
      RC(took.check("rsys_op_ss (target_grad)"));
    }
    return RSYS_OK;
  };
  return hook_finish(run());
}

int32_t rsys_op_shard_rows(int32_t stages, const int32_t* skey, const int32_t* sidx, int32_t N, int32_t V, int32_t* slot, int32_t* uniq,
                           int32_t* tok2u, int32_t* plan, const int32_t* bound, int32_t nb, int32_t* off, float* table, int64_t ld,
                           int32_t table_rows, const int32_t* ids, int32_t sub, float* packed, int32_t n, int32_t D, const int32_t* count,
                           const int32_t* m_matchedid, const int32_t* userid, const int32_t* m_tmid, int32_t Ntok, const float* Frem,
                           int32_t frem_rows, float* x0, int32_t* uid_t, int32_t* tm_t) {
  ARG_CHECK(stages > 0 && stages < 64, "rsys_op_shard_rows: stages is a mask of 1 .. 32");
  const int row_stages = stages & (4 | 8 | 16);
  ARG_CHECK((row_stages & (row_stages - 1)) == 0, "rsys_op_shard_rows: one of the three rows-by-id stages per call");
  std::vector<int> h, h2;
  if (stages & 1) {
    ARG_CHECK(skey && sidx && slot && uniq && tok2u && plan && N >= 1 && N <= (1 << 20) && V >= 0, "rsys_op_shard_rows: plan_unique arguments");
    RC(hook_ints(skey, N, h)); RC(hook_ints(sidx, N, h2));
    for (int p = 0; p < N; ++p) {
      ARG_CHECK(h[p] >= 0 && h[p] <= V && (p == 0 || h[p - 1] <= h[p]), "rsys_op_shard_rows: skey ascending in [0, V]");
      ARG_CHECK(h2[p] >= 0 && h2[p] < N, "rsys_op_shard_rows: sidx in [0, N)");
    }
  }
  if (stages & 2) {
    ARG_CHECK(uniq && plan && bound && off && nb >= 2 && nb <= 64, "rsys_op_shard_rows: plan_offsets arguments");
    if (!(stages & 1)) { RC(hook_ints(plan, 2, h)); ARG_CHECK(h[0] >= 0 && h[0] <= (1 << 20) + 1, "rsys_op_shard_rows: plan[0] = the number of unique slots"); }
  }
  if (row_stages) {
    ARG_CHECK(table && ids && packed && n >= 0 && D >= 4 && D % 4 == 0 && ld >= D && ld % 4 == 0 && table_rows >= 1, "rsys_op_shard_rows: rows-by-id arguments");
    long long live = n, lo = sub;
    if (row_stages == 16) {
      ARG_CHECK(count, "rsys_op_shard_rows: the counted form takes a device count");
      RC(hook_ints(count, 1, h));
      ARG_CHECK(h[0] >= 0, "rsys_op_shard_rows: *count >= 0");
      live = std::min<long long>(n, h[0]); lo = 0;
    }
    RC(hook_ints(ids, live, h));
    for (int id : h) ARG_CHECK(id >= lo && id - lo < table_rows, "rsys_op_shard_rows: an id outside the table");
  }
  if (stages & 32) {
    ARG_CHECK(m_matchedid && userid && m_tmid && Frem && tok2u && plan && x0 && uid_t && tm_t && Ntok >= 1 && D >= 4 && D % 4 == 0 && frem_rows >= 1,
              "rsys_op_shard_rows: gather_items_remote arguments");
    if (!(stages & 1)) {
      RC(hook_ints(tok2u, Ntok, h)); RC(hook_ints(plan, 2, h2));
      for (int u : h) ARG_CHECK(u >= 0 && u < frem_rows, "rsys_op_shard_rows: tok2u outside the fetched rows");
      ARG_CHECK(h2[1] >= 0 && h2[1] < frem_rows, "rsys_op_shard_rows: plan[1] outside the fetched rows");
    } else
      ARG_CHECK(Ntok == N && frem_rows >= N + 1, "rsys_op_shard_rows: with plan_unique, Ntok == N and frem_rows >= N + 1");
  }
  const auto run = [&]() -> int {
    if (stages & 1) RC(launch_plan_unique(skey, sidx, N, V, slot, uniq, tok2u, plan, nullptr));
    if (stages & 2) RC(launch_plan_offsets(uniq, plan, bound, nb, off, nullptr));
    if (stages & 4) RC(launch_gather_rows_by_id(table, ld, ids, sub, packed, n, D, nullptr));
    if (stages & 8) RC(launch_add_rows_by_id(packed, ids, sub, table, ld, n, D, nullptr));
    if (stages & 16) RC(launch_add_rows_by_id_counted(packed, ids, count, table, ld, n, D, nullptr));
    if (stages & 32) {
      BatchDev b{};   // the kernel reads N, m_matchedid, userid and m_tmid
      b.N = Ntok; b.m_matchedid = const_cast<int*>(m_matchedid); b.userid = userid; b.m_tmid = const_cast<int*>(m_tmid);
      RC(launch_gather_items_remote(b, Frem, tok2u, plan, D, x0, uid_t, tm_t, nullptr));
    }
    return RSYS_OK;
  };
  return hook_finish(run());
}

// ---------------------------------------------------------------- the index and compaction kernels on caller-provided buffers
// (compact.hip, the position selection, row movers and column sums of elementwise.hip, the batched transpose of optim.hip).  Each call
// runs the production launcher unchanged on the null stream and synchronises; index arrays that address a caller buffer are copied back
// once and checked before anything is launched.

int32_t rsys_op_select_positions(int32_t form, int32_t ntask, const float* w, int32_t N, int32_t topk, int32_t* idx, float* stats,
                                 int32_t* npos) {
  switches_parse();
  ARG_CHECK(form == 0 || form == 1, "rsys_op_select_positions: form 0 (one workgroup per task) or 1 (chunked)");
  ARG_CHECK(w && idx && stats && npos && ntask >= 1 && ntask <= 4 && N >= 1 && N <= (1 << 24) && topk >= 1 && topk <= N,
            "rsys_op_select_positions: 1..4 tasks, 1 <= topk <= N <= 2^24");
  const float* ws[4]; int* is[4]; float* sts[4]; int* nps[4];
  for (int i = 0; i < ntask; ++i) { ws[i] = w + (long long)i * N; is[i] = idx + (long long)i * topk; sts[i] = stats + 2 * i; nps[i] = npos + i; }
  if (form == 0) return hook_finish(launch_select_positions_batch(ntask, ws, N, topk, is, sts, nps, nullptr));
  HookScratch scratch("rsys_op_select_positions");
  void* chunks = nullptr;
  RC(scratch.alloc(&chunks, 3 * 4 * 32 * 4));   // 3 arrays of 4 tasks x 32 chunks (launch_select_positions_chunked)
  return hook_finish(launch_select_positions_chunked(ntask, ws, N, topk, is, sts, nps, chunks, nullptr));
}

int32_t rsys_op_token_union(int32_t ntask, const int32_t* idx, int32_t cap, const int32_t* npos, int32_t null_mask, int32_t NT, int32_t* bits,
                            int32_t* pre, int32_t* nsel) {
  switches_parse();
  ARG_CHECK(idx && npos && bits && pre && nsel && ntask >= 1 && ntask <= 4 && cap >= 1 && NT >= 1 && null_mask >= 0 && null_mask < 16,
            "rsys_op_token_union: arguments");
  std::vector<int> hn, hi;
  RC(hook_ints(npos, ntask, hn));
  const int* ips[4]; const int* nps[4];
  for (int ti = 0; ti < ntask; ++ti) {
    const bool null_task = (null_mask >> ti) & 1;
    ips[ti] = null_task ? nullptr : idx + (long long)ti * cap; nps[ti] = npos + ti;
    if (null_task) continue;
    ARG_CHECK(hn[ti] >= 0 && hn[ti] <= cap, "rsys_op_token_union: 0 <= npos <= cap");
    RC(hook_ints(idx + (long long)ti * cap, hn[ti], hi));
    for (int i : hi) ARG_CHECK(i >= 0 && 2LL * i + 1 < NT, "rsys_op_token_union: a live position outside [0, NT / 2)");
  }
  return hook_finish(launch_token_union(ips, nps, ntask, NT, (unsigned int*)bits, pre, nsel, nullptr));
}

int32_t rsys_op_selected_first(const int32_t* bits, const int32_t* pre, int32_t B, int32_t T, const int32_t* uid, const int32_t* tm,
                               const int32_t* rope_pos, int32_t* slot, int32_t* sel, int32_t sel_cap, int32_t* perm, int32_t* uid_p,
                               int32_t* tm_p, int32_t* pos_p, int32_t* slot_p, int32_t* sel_p, int32_t* q_active) {
  switches_parse();
  ARG_CHECK(bits && pre && uid && tm && slot && sel && perm && uid_p && tm_p && pos_p && slot_p && sel_p && q_active && B >= 1 && T >= 1 &&
                T <= 4096 && sel_cap >= 0 && (long long)B * T <= (1 << 19),
            "rsys_op_selected_first: arguments (T <= 4096, B T <= 2^19)");
  const long long nw = ((long long)B * T + 31) / 32;
  std::vector<int> hb, hp;
  RC(hook_ints(bits, nw, hb)); RC(hook_ints(pre, nw, hp));
  long long run = 0;   // sel / sel_p are addressed by pre[w] + a count inside word w
  for (long long w = 0; w < nw; ++w) {
    ARG_CHECK(hp[(size_t)w] == run, "rsys_op_selected_first: pre is not the exclusive prefix count of bits");
    run += __builtin_popcount((unsigned)hb[(size_t)w]);
  }
  ARG_CHECK(run <= sel_cap, "rsys_op_selected_first: more selected tokens than sel_cap");
  return hook_finish(launch_selected_first((const unsigned int*)bits, pre, slot, sel, uid, tm, rope_pos, B, T, perm, uid_p, tm_p, pos_p, slot_p, sel_p, q_active, nullptr));
}

int32_t rsys_op_rows(int32_t kind, int32_t dtype, const void* src, int64_t src_rows, void* dst, int64_t dst_rows, int64_t ld, int32_t n, int32_t D,
                     const int32_t* map, int64_t map_len, const int32_t* idx, int32_t parity, const int32_t* count, int32_t Tseq) {
  switches_parse();
  ARG_CHECK(kind >= 0 && kind <= 6, "rsys_op_rows: kind 0 .. 6");
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_rows: dtype fp32 or bf16");
  const bool bf = dtype == RSYS_DTYPE_BF16;
  ARG_CHECK(!bf || (kind != 4 && kind != 6), "rsys_op_rows: the adding movers are fp32 only");
  const int E = bf ? 8 : 4;
  ARG_CHECK(src && dst && src_rows >= 1 && dst_rows >= 1 && dst_rows <= (1 << 24) && src_rows <= (1 << 24) && D >= E && D % E == 0,
            "rsys_op_rows: buffers, at most 2^24 rows each, D a multiple of 16 bytes");
  const bool strided = kind == 0 || kind == 1 || kind == 2 || kind == 5 || kind == 6;
  if (strided) ARG_CHECK(ld >= D && ld % E == 0, "rsys_op_rows: ld >= D, a multiple of 16 bytes");
  ARG_CHECK(parity == 0 || parity == 1, "rsys_op_rows: parity 0 or 1");
  std::vector<int> hm, hi, hc;
  long long live = n;
  if (kind != 0) ARG_CHECK(n >= 1, "rsys_op_rows: n >= 1");
  if (kind == 0) {   // gather_rows_sel: cap = dst_rows
    ARG_CHECK(map && count && map_len >= 0, "rsys_op_rows: gather_rows_sel takes sel and a device count");
    RC(hook_ints(count, 1, hc));
    ARG_CHECK(hc[0] >= 0 && hc[0] <= dst_rows && hc[0] <= map_len, "rsys_op_rows: 0 <= *count <= min(cap, map_len)");
    RC(hook_ints(map, hc[0], hm));
    for (int r : hm) ARG_CHECK(r >= 0 && r < src_rows, "rsys_op_rows: sel outside the source");
  } else if (kind == 1) {   // scatter_rows_fill: n = B batch rows of Tseq places
    ARG_CHECK(map && count && Tseq >= 1 && (long long)n * Tseq == dst_rows && map_len == dst_rows, "rsys_op_rows: scatter_rows_fill takes slot_p [n Tseq] and q_active [n]");
    RC(hook_ints(count, n, hc)); RC(hook_ints(map, map_len, hm));
    for (int b = 0; b < n; ++b) {
      ARG_CHECK(hc[b] >= 0 && hc[b] <= (1 << 20), "rsys_op_rows: q_active >= 0");
      for (long long p = 0; p < std::min<long long>(Tseq, 64LL * hc[b]); ++p) {
        const int s = hm[(size_t)((long long)b * Tseq + p)];
        ARG_CHECK(s >= -1 && s < src_rows, "rsys_op_rows: slot_p outside the compact rows");
      }
    }
  } else if (kind == 2) {   // scatter_rows_map
    ARG_CHECK(map && map_len >= n && src_rows >= n, "rsys_op_rows: scatter_rows_map takes map [n]");
    RC(hook_ints(map, n, hm));
    std::vector<char> seen((size_t)dst_rows, 0);
    for (int r : hm) {
      ARG_CHECK(r >= 0 && r < dst_rows && !seen[(size_t)r], "rsys_op_rows: map outside the destination or not distinct");
      seen[(size_t)r] = 1;
    }
  } else {   // 3 .. 6: head rows, token 2 idx[r] + parity
    ARG_CHECK(idx, "rsys_op_rows: idx");
    const bool via_slot = kind == 3 || kind == 4, adds = kind == 4 || kind == 6;
    if (via_slot) ARG_CHECK(map && map_len >= 1, "rsys_op_rows: the slot forms take slot [map_len]");
    if (kind == 4) ARG_CHECK(count, "rsys_op_rows: scatter_rows_add_slot takes a device count");
    if (adds && count) { RC(hook_ints(count, 1, hc)); ARG_CHECK(hc[0] >= 0, "rsys_op_rows: *count >= 0"); live = std::min<long long>(n, hc[0]); }
    if (adds) ARG_CHECK(src_rows >= n, "rsys_op_rows: src holds n rows");
    else ARG_CHECK(dst_rows >= n, "rsys_op_rows: dst holds n rows");
    RC(hook_ints(idx, live, hi));
    if (via_slot) RC(hook_ints(map, map_len, hm));
    const long long tokens = via_slot ? map_len : (adds ? dst_rows : src_rows), table = adds ? dst_rows : src_rows;
    std::vector<char> seen(adds ? (size_t)table : 0, 0);
    for (int i : hi) {
      const long long tok = 2LL * i + parity;
      ARG_CHECK(i >= 0 && tok < tokens, "rsys_op_rows: a position outside the token range");
      long long row = tok;
      if (via_slot) { row = hm[(size_t)tok]; ARG_CHECK(row >= -1 && row < table, "rsys_op_rows: slot outside the compact rows"); }
      if (adds && row >= 0) { ARG_CHECK(!seen[(size_t)row], "rsys_op_rows: two live rows add to one destination row"); seen[(size_t)row] = 1; }
    }
  }
  const int cap = (int)dst_rows;
  int rc;
  switch (kind) {
    case 0: rc = BY_DTYPE(dtype, launch_gather_rows_sel<Elt>((const Elt*)src, ld, map, count, cap, (Elt*)dst, D, nullptr)); break;
    case 1: rc = BY_DTYPE(dtype, launch_scatter_rows_fill<Elt>((const Elt*)src, map, count, n, Tseq, (Elt*)dst, ld, D, nullptr)); break;
    case 2: rc = BY_DTYPE(dtype, launch_scatter_rows_map<Elt>((const Elt*)src, map, n, (Elt*)dst, ld, D, nullptr)); break;
    case 3: rc = BY_DTYPE(dtype, launch_gather_rows_slot<Elt>((const Elt*)src, map, idx, parity, (Elt*)dst, n, D, nullptr)); break;
    case 4: rc = launch_scatter_rows_add_slot((const float*)src, map, idx, parity, count, (float*)dst, n, D, nullptr); break;
    case 5: rc = BY_DTYPE(dtype, launch_gather_rows<Elt>((const Elt*)src, ld, idx, parity, (Elt*)dst, n, D, nullptr)); break;
    default: rc = launch_scatter_rows_add((const float*)src, idx, parity, (float*)dst, ld, n, D, nullptr, count); break;
  }
  return hook_finish(rc);
}

int32_t rsys_op_colsum(int32_t kind, int32_t deterministic, const float* src, int64_t ld, int64_t rows, int32_t D, float* colsum, void* dst,
                       int64_t ldt) {
  switches_parse();
  ARG_CHECK(kind >= 0 && kind <= 2, "rsys_op_colsum: kind 0 colsum_add, 1 cast_colsum, 2 cast_transpose_colsum");
  ARG_CHECK(src && colsum && rows >= 1 && rows <= (1LL << 24) && D >= 1, "rsys_op_colsum: 1 <= rows <= 2^24");
  if (kind == 0) ARG_CHECK(ld >= D, "rsys_op_colsum: ld >= cols");
  else ARG_CHECK(dst && ld == D, "rsys_op_colsum: the cast forms read a dense source (ld == D) and take dst");
  long long parts;   // the launcher's own grid formula (elementwise.hip)
  if (kind == 0) { const long long rpb = std::max<long long>(64, (rows + 511) / 512); parts = (rows + rpb - 1) / rpb; }
  else if (kind == 1) { const long long rpb = std::max<long long>(32, (rows + 511) / 512); parts = (rows + rpb - 1) / rpb; }
  else { const long long chunks = (rows + 63) / 64, cpb = std::max<long long>(1, (chunks + 2047) / 2048); parts = (chunks + cpb - 1) / cpb; }
  HookScratch scratch("rsys_op_colsum");
  HookDet det(deterministic != 0);
  RC(det.alloc(scratch, parts * D, ceil32(parts) * D));
  RC(hook_finish(kind == 0   ? launch_colsum_add(src, ld, rows, D, colsum, nullptr)
                 : kind == 1 ? launch_cast_colsum(src, (bf16*)dst, rows, D, colsum, nullptr)
                             : launch_cast_transpose_colsum(src, (bf16*)dst, rows, D, ldt, colsum, nullptr)));
  return det.check("rsys_op_colsum");
}

int32_t rsys_op_transpose_bf16(int32_t n_jobs, const void* const* src, void* const* dst, const int32_t* rows, const int32_t* cols,
                               const int64_t* ld_src, const int64_t* ld_dst) {
  switches_parse();
  ARG_CHECK(src && dst && rows && cols && ld_src && ld_dst && n_jobs >= 1 && n_jobs <= 64, "rsys_op_transpose_bf16: 1 .. 64 jobs");
  TransposeBatch b{};
  for (int i = 0; i < n_jobs; ++i) {
    ARG_CHECK(src[i] && dst[i] && ((uintptr_t)src[i] & 15) == 0 && ((uintptr_t)dst[i] & 15) == 0, "rsys_op_transpose_bf16: 16-byte aligned matrices");
    ARG_CHECK(rows[i] >= 1 && cols[i] >= 1 && rows[i] <= (1 << 21) && cols[i] <= (1 << 21), "rsys_op_transpose_bf16: 1 <= rows, cols <= 2^21");
    ARG_CHECK(ld_src[i] >= cols[i] && ld_dst[i] >= rows[i] && ld_src[i] % 8 == 0 && ld_dst[i] % 8 == 0,
              "rsys_op_transpose_bf16: ld_src >= cols, ld_dst >= rows, both multiples of 8 (16-byte row strides)");
    b.job[i] = TransposeJob{src[i], dst[i], rows[i], cols[i], ld_src[i], ld_dst[i]};
  }
  b.n = n_jobs;
  return hook_finish(launch_transpose_bf16(b, nullptr));
}

}  // extern "C"
