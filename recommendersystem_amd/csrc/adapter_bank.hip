// Adapter bank: up to RSYS_ADAPTER_SLOTS rank-8 LoRA adapter sets (q_proj / v_proj, model.py:235-271) held next to the
// frozen trunk of a base model, and the two kernels of the inference forward in which every batch row names the slot it runs with
// (Finetune/embed.py:180-255 serves four adapters on one trunk):
//   stage A   La[t, 0:16]  = xn[t, :] . [A_q; A_v][slot(t)]^T                        (once per layer, reads xn once)
//   stage B   q[t, :]     += rope(2 * La[t, 0:8] . B_q[slot(t)]^T),  v[t, :] += 2 * La[t, 8:16] . B_v[slot(t)]^T   (k is not touched)
// A workgroup works on tokens of ONE batch row (a row is 2S consecutive tokens), so the slot is workgroup-uniform; rows with slot -1
// return before their first load.  Rounding points are those of the finetune model's two LoRA GEMMs (model_forward.hip): operands
// and La in the compute type, fp32 accumulation, alpha = 2 on the fp32 sum, the q part rotated and added to the rotated projection.
// No atomics: every sum has a fixed order.
#include "model_internal.hpp"

namespace rsys {

struct AdapterBank {
  float *A32 = nullptr, *B32 = nullptr;   // fp32 masters: [slots][L][16][D] ([A_q; A_v]) and [slots][L][Nq + Nv][8] (B_q rows, then B_v rows)
  void *A = nullptr, *B = nullptr;        // compute-type copies (bf16 mode; == the masters in fp32 mode)
  void* La = nullptr;                     // [rows_max * 2S][16] compute type: the rank-16 activations of the current layer
  int* d_rows = nullptr;                  // [rows_max] slot per batch row of the current call
  std::vector<unsigned char> have[RSYS_ADAPTER_SLOTS];   // per slot: tensor (4 l + {qA, qB, vA, vB}) has been set since the last clear
  bool any_row = false;                   // the current call names at least one slot
};

static inline int64_t bank_a_floats(const Model* m) { return (int64_t)16 * m->D; }
static inline int64_t bank_b_floats(const Model* m) { return (int64_t)(m->H + m->KV) * m->hd * 8; }

// ------------------------------------------------------------------ kernels
template <typename T> __device__ __forceinline__ void load8(const T* p, float (&v)[8]);
template <> __device__ __forceinline__ void load8<bf16>(const bf16* p, float (&v)[8]) {
  const bf16x8 x = *(const bf16x8*)p;
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = (float)x[k];
}
template <> __device__ __forceinline__ void load8<float>(const float* p, float (&v)[8]) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <typename T> __device__ __forceinline__ void store8(T* p, const float (&v)[8]);
template <> __device__ __forceinline__ void store8<bf16>(bf16* p, const float (&v)[8]) {
  bf16x8 x;
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = (bf16)v[k];
  *(bf16x8*)p = x;
}
template <> __device__ __forceinline__ void store8<float>(float* p, const float (&v)[8]) {
  *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  *(float4*)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// One 16 x 16 MFMA step per wave: tokens on the rows, the 16 LoRA rows on the columns, 16 bytes of each operand row per lane
// straight from global memory (lane l: row l & 15, k offset E * (l >> 4)) -- both operands are row-major with K contiguous.
template <typename T> struct BankMma;
template <> struct BankMma<bf16> {
  static constexpr int KS = 32, E = 8;   // K per step, elements per lane
  using Frag = bf16x8;
  static __device__ __forceinline__ Frag zero() { Frag z; for (int k = 0; k < 8; ++k) z[k] = (bf16)0.f; return z; }
  static __device__ __forceinline__ Frag load(const bf16* p) { return *(const bf16x8*)p; }
  static __device__ __forceinline__ f32x4 mma(Frag a, Frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct BankMma<float> {
  // four 16x16x4 steps on one float4 per lane: step i multiplies element i of both fragments, i.e. k = k0 + 4 * (l >> 4) + i on both
  // sides (the order of k inside a sum does not matter as long as both operands agree)
  static constexpr int KS = 16, E = 4;
  using Frag = float4;
  static __device__ __forceinline__ Frag zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ Frag load(const float* p) { return *(const float4*)p; }
  static __device__ __forceinline__ f32x4 mma(Frag a, Frag b, f32x4 c) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, c, 0, 0, 0);
  }
};

constexpr int BANK_A_TOK = 16;   // tokens per workgroup of stage A (one MFMA tile row block)
constexpr int BANK_B_TOK = 8;    // tokens per workgroup of stage B (2S is a multiple of 8)

// grid (ceil(2S / 16), rows), 256 threads: the four waves split K (wave w takes the K steps w, w + 4, ...), their partial tiles are
// added in wave order through LDS.  Tokens past the row's end (2S % 16 == 8) load zeros and store nothing.
template <typename T>
__global__ __launch_bounds__(256) void adapter_bank_a_kernel(const T* __restrict__ xn, const T* __restrict__ bankA, const int* __restrict__ row_slot,
                                                             int layer, int L, int D, int Ttok, T* __restrict__ La) {
  using MM = BankMma<T>;
  __shared__ float red[4][4][64];
  const int row = blockIdx.y, slot = row_slot[row];
  if (slot < 0) return;
  const int t0 = blockIdx.x * BANK_A_TOK;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const bool tok_ok = t0 + r < Ttok;
  const T* xr = xn + ((long long)row * Ttok + (tok_ok ? t0 + r : 0)) * D;
  const T* ar = bankA + (((long long)slot * L + layer) * 16 + r) * D;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = w * MM::KS; k0 < D; k0 += 4 * MM::KS) {
    const int k = k0 + kq * MM::E;
    const bool k_ok = k < D;   // (D % 16 == 0: a fragment is inside the row or entirely past it)
    const typename MM::Frag xa = (tok_ok && k_ok) ? MM::load(xr + k) : MM::zero();
    const typename MM::Frag ab = k_ok ? MM::load(ar + k) : MM::zero();
    acc = MM::mma(xa, ab, acc);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[w][i][lane] = acc[i];
  __syncthreads();
  // thread (i = wave, lane): element i of lane's accumulator = token 4 * (lane >> 4) + i, LoRA row lane & 15
  const float sum = ((red[0][w][lane] + red[1][w][lane]) + red[2][w][lane]) + red[3][w][lane];
  const int tok = t0 + 4 * kq + w;
  if (tok < Ttok) La[((long long)row * Ttok + tok) * 16 + r] = from_f32<T>(sum);
}

// grid (2S / 8, rows), 256 threads; a work item = 8 consecutive q or v columns of one token (one 16-byte access of bf16 qkv; 8 | hd, so
// the item's RoPE pairs are its own).  The k columns are neither read nor written.
template <typename T>
__global__ __launch_bounds__(256) void adapter_bank_b_kernel(const T* __restrict__ La, const T* __restrict__ bankB, const int* __restrict__ row_slot,
                                                             int layer, int L, int Nq, int Nk, int Nv, int Ttok, int hd,
                                                             const float* __restrict__ rope_cos, const float* __restrict__ rope_sin,
                                                             const int* __restrict__ rope_pos, T* __restrict__ qkv) {
  const int row = blockIdx.y, slot = row_slot[row];
  if (slot < 0) return;
  const int t0 = blockIdx.x * BANK_B_TOK;
  const int ntok = min(BANK_B_TOK, Ttok - t0);
  const int G = (Nq + Nv) >> 3, ld = Nq + Nk + Nv;
  const T* bb = bankB + ((long long)slot * L + layer) * (long long)(Nq + Nv) * 8;
  for (int i = threadIdx.x; i < ntok * G; i += 256) {
    const int tl = i / G, c = (i - tl * G) * 8;
    const bool isq = c < Nq;
    const long long t = (long long)row * Ttok + t0 + tl;
    float la[8], u[8], old[8];
    load8<T>(La + t * 16 + (isq ? 0 : 8), la);
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      float b[8];
      load8<T>(bb + (long long)(c + o) * 8, b);
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = fmaf(la[k], b[k], acc);
      u[o] = 2.f * acc;   // lora_scaling = alpha / rank = 16 / 8
    }
    if (isq) {   // interleaved pairs (model.py:182-190), as the QKV epilogue rotates them
      const int pos = rope_pos ? rope_pos[t] : t0 + tl;
      const int d2 = (c & (hd - 1)) >> 1;
      const float* cs = rope_cos + pos * (hd >> 1) + d2;
      const float* sn = rope_sin + pos * (hd >> 1) + d2;
#pragma unroll
      for (int k = 0; k < 8; k += 2) {
        const float cc = cs[k >> 1], ss = sn[k >> 1];
        const float a0 = u[k] * cc - u[k + 1] * ss, a1 = u[k] * ss + u[k + 1] * cc;
        u[k] = a0; u[k + 1] = a1;
      }
    }
    T* dst = qkv + t * ld + (isq ? c : c + Nk);
    load8<T>(dst, old);
#pragma unroll
    for (int k = 0; k < 8; ++k) u[k] += old[k];
    store8<T>(dst, u);
  }
}

// ------------------------------------------------------------------ bank storage
static int bank_check_model(const Model* m) {
  ARG_CHECK(!m->cfg.finetune, "adapter bank: a finetune = 1 model owns one adapter as its trainable parameters; the bank lives on a base model");
  ARG_CHECK(!m->fp8, "adapter bank: fp8 is pretraining-only (no LoRA on the float8 trunk)");
  return RSYS_OK;
}

static int bank_ensure(Model* m) {
  if (m->bank) return RSYS_OK;
  HIP_CHECK(hipSetDevice(m->device));
  AdapterBank* b = new AdapterBank();
  m->bank = b;   // (model_destroy frees the struct; the device buffers are in m->allocs)
  const int64_t na = (int64_t)RSYS_ADAPTER_SLOTS * m->L * bank_a_floats(m), nb = (int64_t)RSYS_ADAPTER_SLOTS * m->L * bank_b_floats(m);
  DALLOC(b->A32, na * 4); DALLOC(b->B32, nb * 4);
  if (m->bf16_mode) { DALLOC(b->A, na * 2); DALLOC(b->B, nb * 2); } else { b->A = b->A32; b->B = b->B32; }
  DALLOC(b->d_rows, (int64_t)m->rows_max * 4);
  for (int s = 0; s < RSYS_ADAPTER_SLOTS; ++s) b->have[s].assign((size_t)4 * m->L, 0);
  return RSYS_OK;
}

void adapter_bank_free(Model* m) { delete m->bank; m->bank = nullptr; }

// "transformers.layers.{l}.attn.{q,v}_proj_lora_{A,B}.weight" -> layer, which (0 qA, 1 qB, 2 vA, 3 vB)
static bool bank_parse_name(const Model* m, const char* name, int* layer, int* which) {
  int l = -1, used = 0; char proj = 0, mat = 0;
  if (sscanf(name, "transformers.layers.%d.attn.%c_proj_lora_%c.weight%n", &l, &proj, &mat, &used) != 3) return false;
  if (used == 0 || name[used] != 0 || l < 0 || l >= m->L || (proj != 'q' && proj != 'v') || (mat != 'A' && mat != 'B')) return false;
  if (std::string(name) != "transformers.layers." + std::to_string(l) + ".attn." + proj + "_proj_lora_" + mat + ".weight") return false;   // ("+3", " 3": one spelling per tensor)
  *layer = l; *which = (proj == 'v' ? 2 : 0) + (mat == 'B' ? 1 : 0);
  return true;
}

// where tensor `which` of (slot, layer) lives in the masters, and its element count (A: 8 x D; B_q: H hd x 8; B_v: KV hd x 8)
static void bank_locate(const Model* m, int slot, int layer, int which, bool* in_b, int64_t* off, int64_t* n) {
  const int64_t Nq = (int64_t)m->H * m->hd, Nv = (int64_t)m->KV * m->hd;
  const int64_t sl = (int64_t)slot * m->L + layer;
  *in_b = (which & 1) != 0;
  if (!*in_b) { *off = sl * bank_a_floats(m) + (which == 2 ? (int64_t)8 * m->D : 0); *n = (int64_t)8 * m->D; }
  else { *off = sl * bank_b_floats(m) + (which == 3 ? Nq * 8 : 0); *n = (which == 3 ? Nv : Nq) * 8; }
}

int adapter_io(Model* m, int slot, const char* name, float* out, const float* in, int64_t n) {
  RC(bank_check_model(m));
  ARG_CHECK(slot >= 0 && slot < RSYS_ADAPTER_SLOTS, "adapter slot must be in [0, RSYS_ADAPTER_SLOTS)");
  int layer, which;
  if (!bank_parse_name(m, name, &layer, &which)) { set_error(std::string("unknown adapter tensor: ") + name); return RSYS_ERR_ARG; }
  bool in_b; int64_t off, cnt;
  bank_locate(m, slot, layer, which, &in_b, &off, &cnt);
  ARG_CHECK(n == cnt, "element count does not match the adapter tensor's shape");
  if (out) ARG_CHECK(m->bank != nullptr && m->bank->have[slot][4 * layer + which], "adapter tensor has not been set in this slot");
  RC(bank_ensure(m));
  AdapterBank* b = m->bank;
  HIP_CHECK(hipSetDevice(m->device));
  HIP_CHECK(hipStreamSynchronize(m->stream));
  float* master = (in_b ? b->B32 : b->A32) + off;
  if (out) { HIP_CHECK(hipMemcpy(out, master, (size_t)cnt * 4, hipMemcpyDeviceToHost)); return RSYS_OK; }
  HIP_CHECK(hipMemcpy(master, in, (size_t)cnt * 4, hipMemcpyHostToDevice));
  if (m->bf16_mode) {
    RC(launch_cast<bf16>(master, (bf16*)(in_b ? b->B : b->A) + off, cnt, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
  }
  b->have[slot][4 * layer + which] = 1;
  return RSYS_OK;   // (no parameter of the trunk changed: table_dirty / wt_dirty stay as they are)
}

static bool bank_complete(const Model* m, int slot) {
  if (!m->bank) return false;
  for (unsigned char h : m->bank->have[slot]) if (!h) return false;
  return true;
}

int adapter_clear(Model* m, int slot) {
  RC(bank_check_model(m));
  ARG_CHECK(slot >= 0 && slot < RSYS_ADAPTER_SLOTS, "adapter slot must be in [0, RSYS_ADAPTER_SLOTS)");
  if (!m->bank) return RSYS_OK;
  AdapterBank* b = m->bank;
  HIP_CHECK(hipSetDevice(m->device));
  HIP_CHECK(hipStreamSynchronize(m->stream));
  const int64_t na = (int64_t)m->L * bank_a_floats(m), nb = (int64_t)m->L * bank_b_floats(m);
  HIP_CHECK(hipMemset(b->A32 + slot * na, 0, (size_t)na * 4)); HIP_CHECK(hipMemset(b->B32 + slot * nb, 0, (size_t)nb * 4));
  if (m->bf16_mode) { HIP_CHECK(hipMemset((bf16*)b->A + slot * na, 0, (size_t)na * 2)); HIP_CHECK(hipMemset((bf16*)b->B + slot * nb, 0, (size_t)nb * 2)); }
  std::fill(b->have[slot].begin(), b->have[slot].end(), 0);
  return RSYS_OK;
}

int adapter_slots(Model* m, int32_t* mask_out) {
  RC(bank_check_model(m));
  ARG_CHECK(mask_out != nullptr, "null mask");
  int32_t mask = 0;
  for (int s = 0; s < RSYS_ADAPTER_SLOTS; ++s) if (bank_complete(m, s)) mask |= 1 << s;
  *mask_out = mask;
  return RSYS_OK;
}

// ------------------------------------------------------------------ the inference call's side
// checks row_adapter[0 .. rows) and makes it the slot vector of the next forward_trunk (m->bank_rows); adapter_unbind_rows ends that
int adapter_bind_rows(Model* m, const int32_t* row_adapter) {
  RC(bank_check_model(m));
  ARG_CHECK(row_adapter != nullptr, "row_adapter is null (use rsys_infer_select for the base model)");
  ARG_CHECK(m->cur_rows > 0, "no batch uploaded");
  bool any = false;
  for (int r = 0; r < m->cur_rows; ++r) {
    const int s = row_adapter[r];
    ARG_CHECK(s >= -1 && s < RSYS_ADAPTER_SLOTS, "row_adapter entries must be in [-1, RSYS_ADAPTER_SLOTS)");
    if (s >= 0) { ARG_CHECK(bank_complete(m, s), "row_adapter names a slot that is not complete (4 tensors per layer since its last clear)"); any = true; }
  }
  m->bank_rows = nullptr;
  if (!any) return RSYS_OK;   // every row runs the base model: the forward launches what rsys_infer_select launches
  AdapterBank* b = m->bank;
  HIP_CHECK(hipSetDevice(m->device));
  if (!b->La) DALLOC(b->La, (int64_t)m->rows_max * m->T * 16 * m->esz);
  HIP_CHECK(hipMemcpyAsync(b->d_rows, row_adapter, (size_t)m->cur_rows * 4, hipMemcpyHostToDevice, m->stream));
  m->bank_rows = b->d_rows;
  return RSYS_OK;
}
void adapter_unbind_rows(Model* m) { m->bank_rows = nullptr; }

template <typename T>
int adapter_bank_stage_a(Model* m, int l, const T* xn) {
  const AdapterBank* b = m->bank;
  const int rows = m->cur_rows;
  tic(m, "hbm_adapter_bank_a", (double)sizeof(T) * rows * m->T * (m->D + 16.0));
  hipLaunchKernelGGL((adapter_bank_a_kernel<T>), dim3((m->T + BANK_A_TOK - 1) / BANK_A_TOK, rows), dim3(256), 0, m->stream, xn, (const T*)b->A,
                     m->bank_rows, l, m->L, m->D, m->T, (T*)b->La);
  HIP_CHECK(hipGetLastError());
  toc(m);
  return RSYS_OK;
}
template <typename T>
int adapter_bank_stage_b(Model* m, int l, T* qkv, const int* rope_pos) {
  const AdapterBank* b = m->bank;
  const int rows = m->cur_rows, Nq = m->H * m->hd, Nk = m->KV * m->hd;
  tic(m, "hbm_adapter_bank_b", (double)sizeof(T) * rows * m->T * (2.0 * (Nq + Nk) + 16.0));
  hipLaunchKernelGGL((adapter_bank_b_kernel<T>), dim3((m->T + BANK_B_TOK - 1) / BANK_B_TOK, rows), dim3(256), 0, m->stream, (const T*)b->La,
                     (const T*)b->B, m->bank_rows, l, m->L, Nq, Nk, Nk, m->T, m->hd, m->rope_cos, m->rope_sin, rope_pos, qkv);
  HIP_CHECK(hipGetLastError());
  toc(m);
  return RSYS_OK;
}
template int adapter_bank_stage_a<float>(Model*, int, const float*);
template int adapter_bank_stage_a<bf16>(Model*, int, const bf16*);
template int adapter_bank_stage_b<float>(Model*, int, float*, const int*);
template int adapter_bank_stage_b<bf16>(Model*, int, bf16*, const int*);

}  // namespace rsys
