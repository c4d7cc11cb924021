// Adapter bank: up to RSYS_ADAPTER_SLOTS rank-8 LoRA adapter sets (q_proj / v_proj, model.py:235-271) held next to the
// frozen trunk of a base model, and the two kernels of the inference forward in which every batch row names the slot it runs with
// (Finetune/embed.py:180-255 serves four adapters on one trunk):
//   stage A   La[t, 0:16]  = xn[t, :] . [A_q; A_v][slot(t)]^T                        (once per layer, reads xn once)
//   stage B   q[t, :]     += rope(2 * La[t, 0:8] . B_q[slot(t)]^T),  v[t, :] += 2 * La[t, 8:16] . B_v[slot(t)]^T   (k is not touched)
// A workgroup works on tokens of ONE batch row (a row is 2S consecutive tokens) and, 16 | 64, of one 64-token tile of it, so the slot is
// workgroup-uniform; a workgroup whose slot is -1 returns before its first load.  There is ONE kernel per stage.  Where its workgroup
// finds the slot, or the tokens it sums over, is a by-value BankLookup: the slot of the row; or, on packed rows (DESIGN 4zb serving, 4zc
// finetune: several users per row, segments of whole 64-token tiles), the slot of the TILE, with the partial gradients taken per SEGMENT
// and summed per slot in descriptor order.  Rounding points are those of the finetune model's two LoRA GEMMs (model_forward.hip): operands
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
  int* d_tiles = nullptr;                 // [rows_max][ceil(Ta / 64)] slot per 64-token tile of the current call (packed rows)
  std::vector<int32_t> h_tiles;           // its host image in the resident rows' geometry (the source of a stream-ordered copy)
  // ---- training through the bank (allocated by rsys_adapter_train_enable)
  bool train = false;
  float dropout = 0.f;                    // nn.Dropout(p) on the LoRA input, training passes only
  bool drop_now = false;                  // the current pass draws masks (keyed on m->drop_seed, m->drop_step, layer, element)
  float *gA = nullptr, *gB = nullptr;     // fp32 gradients in the masters' layouts
  float *mA = nullptr, *vA = nullptr, *mB = nullptr, *vB = nullptr;   // AdamW moments, same layouts
  int step[RSYS_ADAPTER_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};            // per-slot step count (bias correction)
  void* La_l = nullptr;                   // [L][rows_max * 2S][16] compute type: La of every layer, kept for the backward
  void* dLa = nullptr;                    // [rows_max * 2S][16] compute type: of the layer the backward is in
  float *partA = nullptr, *partB = nullptr;   // per-row partial gradients of that layer: [rows_max][16][D], [rows_max][Nq + Nv][8]
  int* d_task = nullptr;                  // [rows_max] task per batch row of the current call
  float* d_norms = nullptr;               // [RSYS_ADAPTER_SLOTS] the optimizer step's per-slot gradient norms
  // ---- training on packed rows (allocated by the first rsys_adapter_forward_backward_packed)
  int* d_tile_task = nullptr;             // [rows_max][ceil(Ta / 64)] task per tile (the slot map is d_tiles)
  int* d_segs = nullptr;                  // [rows_max * ceil(Ta / 64)][5] the call's segment table
  int n_seg = 0;                          // its length in the current call
  std::vector<int32_t> h_pack;            // host image of (tile slots | tile tasks | segments): rewritten once the stream has passed the last copy
  float *segA = nullptr, *segB = nullptr; // per-segment partial gradients [seg_cap][16][D], [seg_cap][Nq + Nv][8]: grown to the call's segment count
  int seg_cap = 0;
};

struct BankLaunch {                       // the plain arguments of one layer's bank launches
  int rows, Ttok, D, H, KV, hd, L, layer;
  const int* row_slot;                    // [rows] device
  const int* tile_slot = nullptr;         // [rows][ceil(Ttok / 64)] device: the stages read it instead of row_slot when set
  const int* segs = nullptr;              // [n_seg][5] device (row, first column, columns, slot, task): with tile_slot, the backward's partials and sums
  int n_seg = 0;
  const void *bankA, *bankB;              // compute type: [slots][L][16][D], [slots][L][Nq + Nv][8]
  float p; unsigned long long seed; unsigned int stream;   // dropout key (a_train, da, dx)
  hipStream_t s;
};

static inline int64_t bank_a_floats(const Model* m) { return (int64_t)16 * m->D; }
static inline int64_t bank_b_floats(const Model* m) { return (int64_t)(m->H + m->KV) * m->hd * 8; }
template <typename T> static inline T* bank_la(const Model* m, int l) { return (T*)m->bank->La_l + (int64_t)l * m->rows_max * m->Ta * 16; }   // layer l's La of a training pass

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

constexpr int BANK_A_TOK = 16;   // tokens per workgroup of stage A and dLa (one MFMA tile row block)
constexpr int BANK_B_TOK = 8;    // tokens per workgroup of stage B and dx (2S is a multiple of 8)

// What a workgroup works for.  It reads blockIdx and kernel arguments alone, so it stays in scalar registers.
//   token stages (a, b, dla, dx)   nt == 0: map [rows], the slot of the row;  nt > 0: map [rows][nt], nt = ceil(Ttok / 64), the slot of the
//                                  64-token tile the workgroup's 16 or 8 tokens lie in (packed rows)
//   partials (da, db), grid.y = the units:  segs == nullptr: unit = batch row, all its tokens, skipped when map[row] < 0;  otherwise unit
//                                  = a segment of segs [n_seg][5] = (row, first column, columns, slot, task): its whole 64-token tiles, tokens
//                                  [2 c0, min(Ttok, 2 c0 + 64 ceil(columns / 32))), which nobody else owns; skipped when its slot < 0
struct BankLookup {
  const int* map; int nt; const int* segs;
  __device__ __forceinline__ int slot(int row, int t0) const { return map[nt ? row * nt + (t0 >> 6) : row]; }
  __device__ __forceinline__ bool unit(int Ttok, int* row, int* kb, int* ke) const {
    if (!segs) { *row = blockIdx.y; *kb = 0; *ke = Ttok; return map[blockIdx.y] >= 0; }
    const int* sg = segs + (long long)blockIdx.y * 5;
    *row = sg[0]; *kb = 2 * sg[1];
    *ke = min(Ttok, *kb + 64 * ((sg[2] + 31) >> 5));
    return sg[3] >= 0;
  }
};

// ---- training through the bank
// nn.Dropout of the LoRA input (model.py:238,265,269) drawn where it is used instead of in a pass of its own: element e of the layer's
// [tokens][D] input is kept iff u01(Philox(seed)(e >> 2, stream)[e & 3]) >= p -- launch_dropout's mask, with stream = step * 64 + layer.
// The forward (stage A) and the two backward kernels that need drop(xn) or drop' call the same function with the same key.
struct BankDrop {
  float p, keep; Philox ph; unsigned int stream;
  __device__ BankDrop(float p_, unsigned long long seed, unsigned int stream_) : p(p_), keep(1.f / (1.f - p_)), ph(seed), stream(stream_) {}
  // mask factors (keep or 0) of the 4 elements [4 q, 4 q + 4)
  __device__ __forceinline__ void quad(long long q, float (&f)[4]) const {
    uint32_t r[4];
    ph.gen((unsigned long long)q, stream, r);
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = u01(r[k]) >= p ? keep : 0.f;
  }
  __device__ __forceinline__ float one(long long e) const {
    uint32_t r[4];
    ph.gen((unsigned long long)(e >> 2), stream, r);
    return u01(r[e & 3]) >= p ? keep : 0.f;
  }
};
struct BankNoDrop { __device__ BankNoDrop(float, unsigned long long, unsigned int) {} };   // (stage A of the inference forward: no key, no Philox)
// drop(x) of one fragment of E consecutive elements starting at element e0 (a multiple of 4), rounded to T as launch_dropout stores it
__device__ __forceinline__ bf16x8 bank_drop_frag(bf16x8 x, long long e0, const BankDrop& dr) {
  float f0[4], f1[4];
  dr.quad(e0 >> 2, f0); dr.quad((e0 >> 2) + 1, f1);
#pragma unroll
  for (int k = 0; k < 4; ++k) { x[k] = (bf16)((float)x[k] * f0[k]); x[4 + k] = (bf16)((float)x[4 + k] * f1[k]); }
  return x;
}
__device__ __forceinline__ float4 bank_drop_frag(float4 x, long long e0, const BankDrop& dr) {
  float f[4];
  dr.quad(e0 >> 2, f);
  return make_float4(x.x * f[0], x.y * f[1], x.z * f[2], x.w * f[3]);
}
// E elements `stride` apart as one fragment (operands whose contraction index is not the contiguous one)
__device__ __forceinline__ bf16x8 bank_gather(const bf16* p, long long stride) {
  bf16x8 x;
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = p[k * stride];
  return x;
}
__device__ __forceinline__ float4 bank_gather(const float* p, long long stride) { return make_float4(p[0], p[stride], p[2 * stride], p[3 * stride]); }
__device__ __forceinline__ void bank_frag_mul(bf16x8& x, int k, float f) { x[k] = (bf16)((float)x[k] * f); }
__device__ __forceinline__ void bank_frag_mul(float4& x, int k, float f) { ((float*)&x)[k] *= f; }

// Stage A.  grid (ceil(2S / 16), rows), 256 threads: the four waves split K (wave w takes the K steps w, w + 4, ...), their partial tiles
// are added in wave order through LDS.  Tokens past the row's end (2S % 16 == 8) load zeros and store nothing.  DROP = false is the
// inference forward; DROP = true a training pass: the LoRA input under the dropout mask of key (p, seed, stream) (p == 0: the same sums),
// written to the layer's own La.
template <typename T, bool DROP>
__global__ __launch_bounds__(256) void adapter_bank_a_kernel(const T* __restrict__ xn, const T* __restrict__ bankA, BankLookup look, int layer, int L, int D,
                                                             int Ttok, T* __restrict__ La, float p, unsigned long long seed, unsigned int stream) {
  using MM = BankMma<T>;
  __shared__ float red[4][4][64];
  const int row = blockIdx.y, t0 = blockIdx.x * BANK_A_TOK, slot = look.slot(row, t0);
  if (slot < 0) return;
  const typename std::conditional<DROP, BankDrop, BankNoDrop>::type dr(p, seed, stream);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const bool tok_ok = t0 + r < Ttok;
  const long long tok = (long long)row * Ttok + (tok_ok ? t0 + r : 0);
  const T* xr = xn + tok * D;
  const T* ar = bankA + (((long long)slot * L + layer) * 16 + r) * D;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = w * MM::KS; k0 < D; k0 += 4 * MM::KS) {
    const int k = k0 + kq * MM::E;
    const bool k_ok = k < D;   // (D % 16 == 0: a fragment is inside the row or entirely past it)
    typename MM::Frag xa = (tok_ok && k_ok) ? MM::load(xr + k) : MM::zero();
    if constexpr (DROP) {
      if (p > 0.f && tok_ok && k_ok) xa = bank_drop_frag(xa, tok * D + k, dr);
    }
    const typename MM::Frag ab = k_ok ? MM::load(ar + k) : MM::zero();
    acc = MM::mma(xa, ab, acc);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[w][i][lane] = acc[i];
  __syncthreads();
  // thread (i = wave, lane): element i of lane's accumulator = token 4 * (lane >> 4) + i, LoRA row lane & 15
  const float sum = ((red[0][w][lane] + red[1][w][lane]) + red[2][w][lane]) + red[3][w][lane];
  const int tk = t0 + 4 * kq + w;
  if (tk < Ttok) La[((long long)row * Ttok + tk) * 16 + r] = from_f32<T>(sum);
}

// Stage B.  grid (2S / 8, rows), 256 threads; a work item = 8 consecutive q or v columns of one token (one 16-byte access of bf16 qkv;
// 8 | hd, so the item's RoPE pairs are its own).  The k columns are neither read nor written.
template <typename T>
__global__ __launch_bounds__(256) void adapter_bank_b_kernel(const T* __restrict__ La, const T* __restrict__ bankB, BankLookup look, int layer, int L, int Nq,
                                                             int Nk, int Nv, int Ttok, int hd, const float* __restrict__ rope_cos,
                                                             const float* __restrict__ rope_sin, const int* __restrict__ rope_pos, T* __restrict__ qkv) {
  const int row = blockIdx.y, t0 = blockIdx.x * BANK_B_TOK, slot = look.slot(row, t0);
  if (slot < 0) return;
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

// dLa[t, 0:8] = 2 dq_t . B_q[slot], dLa[t, 8:16] = 2 dv_t . B_v[slot] (the un-rotated dqkv the finetune model's gemm_lora_dla reads; rounded
// to the compute type as that GEMM stores it).  grid (ceil(2S / 16), rows), 256 threads: stage A's tile -- tokens on the rows, the 16
// LoRA columns on the columns -- with K = the q columns, then the v columns; B is [column][8], so its fragment is gathered 8 apart and
// is zero on the half of the LoRA columns the segment does not feed.  The four waves split the K steps, partial tiles added in wave order.
template <typename T>
__global__ __launch_bounds__(256) void adapter_bank_dla_kernel(const T* __restrict__ dqkv, const T* __restrict__ bankB, BankLookup look, int layer, int L,
                                                               int Nq, int Nk, int Nv, int Ttok, T* __restrict__ dLa) {
  using MM = BankMma<T>;
  __shared__ float red[4][4][64];
  const int row = blockIdx.y, t0 = blockIdx.x * BANK_A_TOK, slot = look.slot(row, t0);
  if (slot < 0) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const bool tok_ok = t0 + r < Ttok;
  const int ld = Nq + Nk + Nv;
  const T* gr = dqkv + ((long long)row * Ttok + (tok_ok ? t0 + r : 0)) * ld;
  const T* bb = bankB + ((long long)slot * L + layer) * (long long)(Nq + Nv) * 8;
  const int sq = (Nq + MM::KS - 1) / MM::KS, sv = (Nv + MM::KS - 1) / MM::KS;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int st = w; st < sq + sv; st += 4) {
    const bool isq = st < sq;
    const int k = (isq ? st : st - sq) * MM::KS + kq * MM::E;   // column inside the segment (8 | Nq, Nv: a fragment is inside or past it)
    const bool k_ok = k < (isq ? Nq : Nv);
    const typename MM::Frag ga = (tok_ok && k_ok) ? MM::load(gr + (isq ? k : Nq + Nk + k)) : MM::zero();
    const bool mine = isq ? r < 8 : r >= 8;                     // this lane's LoRA column is fed by this segment
    const typename MM::Frag bf = (k_ok && mine) ? bank_gather(bb + (long long)(isq ? k : Nq + k) * 8 + (r & 7), 8) : MM::zero();
    acc = MM::mma(ga, bf, acc);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[w][i][lane] = acc[i];
  __syncthreads();
  const float sum = ((red[0][w][lane] + red[1][w][lane]) + red[2][w][lane]) + red[3][w][lane];
  const int tk = t0 + 4 * kq + w;
  if (tk < Ttok) dLa[((long long)row * Ttok + tk) * 16 + r] = from_f32<T>(2.f * sum);   // lora_scaling = 2 on the fp32 sum
}

// dxn[t, :] += drop'(dLa[t, :] . [A_q; A_v][slot]) (K = 16: no MFMA).  grid (2S / 8, rows), 256 threads, an item = 8 columns of one
// token.  Rounding as the finetune model's gemm_lora_dx: without dropout the fp32 sum is added to dxn; with it the sum is rounded to the
// compute type first (that model stores it), masked and scaled, then added.
template <typename T>
__global__ __launch_bounds__(256) void adapter_bank_dx_kernel(const T* __restrict__ dLa, const T* __restrict__ bankA, BankLookup look, int layer, int L, int D,
                                                              int Ttok, T* __restrict__ dxn, float p, unsigned long long seed, unsigned int stream) {
  const int row = blockIdx.y, t0 = blockIdx.x * BANK_B_TOK, slot = look.slot(row, t0);
  if (slot < 0) return;
  const BankDrop dr(p, seed, stream);
  const int ntok = min(BANK_B_TOK, Ttok - t0);
  const int G = D >> 3;
  const T* aa = bankA + ((long long)slot * L + layer) * 16 * (long long)D;
  for (int i = threadIdx.x; i < ntok * G; i += 256) {
    const int tl = i / G, c = (i - tl * G) * 8;
    const long long t = (long long)row * Ttok + t0 + tl;
    float g0[8], g1[8], u[8], old[8];
    load8<T>(dLa + t * 16, g0); load8<T>(dLa + t * 16 + 8, g1);
#pragma unroll
    for (int k = 0; k < 8; ++k) u[k] = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      float a[8];
      load8<T>(aa + (long long)j * D + c, a);
      const float g = j < 8 ? g0[j] : g1[j - 8];
#pragma unroll
      for (int k = 0; k < 8; ++k) u[k] = fmaf(g, a[k], u[k]);
    }
    if (p > 0.f) {
      float f0[4], f1[4];
      const long long e0 = t * D + c;
      dr.quad(e0 >> 2, f0); dr.quad((e0 >> 2) + 1, f1);
#pragma unroll
      for (int k = 0; k < 4; ++k) { u[k] = to_f32(from_f32<T>(u[k])) * f0[k]; u[4 + k] = to_f32(from_f32<T>(u[4 + k])) * f1[k]; }
    }
    T* dst = dxn + t * D + c;
    load8<T>(dst, old);
#pragma unroll
    for (int k = 0; k < 8; ++k) u[k] += old[k];
    store8<T>(dst, u);
  }
}

// Partial of dA per unit (BankLookup: a batch row, or a segment): partA[unit][j][d] = sum over the unit's tokens t, ascending, of
// dLa[t][j] drop(xn)[t][d].  grid (ceil(D / 64), units), 256 threads: every wave owns 16 columns d and the whole contraction (K = the
// unit's tokens), so a partial has one fixed order and no cross-wave sum.  MFMA tile: the 16 LoRA rows j on the rows, d on the columns;
// both operands have the token as their OUTER index, so the fragments are gathered (16 resp. D apart).
template <typename T>
__global__ __launch_bounds__(256) void adapter_bank_da_kernel(const T* __restrict__ dLa, const T* __restrict__ xn, BankLookup look, int D, int Ttok,
                                                              float* __restrict__ partA, float p, unsigned long long seed, unsigned int stream) {
  using MM = BankMma<T>;
  int row, kb, ke;   // the contraction runs over tokens [kb, ke) of `row`, kb a multiple of 64
  if (!look.unit(Ttok, &row, &kb, &ke)) return;
  float* dst = partA + (long long)blockIdx.y * 16 * D;
  const BankDrop dr(p, seed, stream);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int d0 = (blockIdx.x * 4 + w) * 16;
  if (d0 >= D) return;   // (D % 16 == 0; no barrier below)
  const int r = lane & 15, kq = lane >> 4;
  const long long tb = (long long)row * Ttok;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = kb; k0 < ke; k0 += MM::KS) {
    const int k = k0 + kq * MM::E;
    const bool k_ok = k < ke;   // (2S % 8 == 0: a fragment's tokens are inside the range or all past it)
    typename MM::Frag ga = MM::zero(), xb = MM::zero();
    if (k_ok) {
      ga = bank_gather(dLa + (tb + k) * 16 + r, 16);
      xb = bank_gather(xn + (tb + k) * D + d0 + r, D);
      if (p > 0.f) {
#pragma unroll
        for (int i = 0; i < MM::E; ++i) bank_frag_mul(xb, i, dr.one((tb + k + i) * D + d0 + r));
      }
    }
    acc = MM::mma(ga, xb, acc);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) dst[(long long)(4 * kq + i) * D + d0 + r] = acc[i];
}

// Partial of dB per unit: partB[unit][c][j] = sum over the unit's tokens, ascending, of dqv[t][c] La[t][j (q columns) | 8 + j (v columns)]
// (the factor 2 is applied when the units are added).  grid (ceil((Nq + Nv) / 64), units), 256 threads; a wave owns 16 columns c of
// [dq | dv] and the whole contraction; the tile's 16 columns are La's, of which a q (v) row keeps the first (last) 8.
template <typename T>
__global__ __launch_bounds__(256) void adapter_bank_db_kernel(const T* __restrict__ dqkv, const T* __restrict__ La, BankLookup look, int Nq, int Nk, int Nv,
                                                              int Ttok, float* __restrict__ partB) {
  using MM = BankMma<T>;
  int row, kb, ke;
  if (!look.unit(Ttok, &row, &kb, &ke)) return;
  float* dst = partB + (long long)blockIdx.y * (Nq + Nv) * 8;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c0 = (blockIdx.x * 4 + w) * 16;
  if (c0 >= Nq + Nv) return;
  const int r = lane & 15, kq = lane >> 4;
  const int ld = Nq + Nk + Nv;
  const long long tb = (long long)row * Ttok;
  const int ca = c0 + r;                              // this lane's row of the tile as the A operand
  const bool ca_ok = ca < Nq + Nv;
  const int col = ca < Nq ? ca : ca + Nk;            // its column of dqkv
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = kb; k0 < ke; k0 += MM::KS) {
    const int k = k0 + kq * MM::E;
    const bool k_ok = k < ke;
    const typename MM::Frag ga = (k_ok && ca_ok) ? bank_gather(dqkv + (tb + k) * ld + col, ld) : MM::zero();
    const typename MM::Frag lb = k_ok ? bank_gather(La + (tb + k) * 16 + r, 16) : MM::zero();
    acc = MM::mma(ga, lb, acc);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + 4 * kq + i;
    if (c >= Nq + Nv) continue;
    const bool isq = c < Nq;
    if (isq ? r < 8 : r >= 8) dst[(long long)c * 8 + (r & 7)] = acc[i];
  }
}

// g[slot][layer][e] += alpha * (sum of part[u][e] over the units u of `slot`, ascending): one thread per element, the fixed order that
// makes a call reproducible and a slot's gradient independent of the other slots' units.  key[u * STRIDE] is unit u's slot: row_slot with
// STRIDE 1, or the segment table from its slot field on with STRIDE 5 (descriptor order).  A slot without a unit is not touched.
// (STRIDE is a template parameter, not an argument: with a run-time stride the compiler no longer unrolls the row form's key loop by 8,
// and the unpacked joint step measured 0.09 ms of 18.8 slower, outside the parent's spread -- DESIGN 4zc.)
template <int STRIDE>
__global__ __launch_bounds__(256) void adapter_bank_reduce_kernel(const float* __restrict__ part, const int* __restrict__ key, int units, long long n,
                                                                  float alpha, float* __restrict__ g, long long slot_stride) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  for (int a = 0; a < RSYS_ADAPTER_SLOTS; ++a) {
    float acc = 0.f; bool any = false;
    for (int u = 0; u < units; ++u)
      if (key[u * STRIDE] == a) { acc += part[(long long)u * n + e]; any = true; }
    if (any) g[(long long)a * slot_stride + e] += alpha * acc;
  }
}

// The bank's optimizer step (clip_grad_norm_ + AdamW.step + zero_grad of train.py:273-275 per adapter): one workgroup of 1024 threads
// per slot.  Phase 1: the slot's sum of squared gradients, A tensors then B tensors, every thread its strided share in ascending
// order, then one fixed tree -- the slot's own global norm.  Phase 2: g * min(1, max_norm / (norm + 1e-6)), the AdamW update of
// optim.hip's adamw_kernel (decoupled decay on every tensor: all LoRA tensors are 2-D), zeroed gradient, refreshed compute-type copy.
struct BankStepRec { int active; float lr, max_norm, bc1, bc2_sqrt; };
struct BankStepArgs { BankStepRec rec[RSYS_ADAPTER_SLOTS]; };
template <typename T>
__global__ __launch_bounds__(1024) void adapter_bank_adamw_kernel(float* A32, float* B32, float* gA, float* gB, float* mA, float* vA, float* mB, float* vB,
                                                                  T* A, T* B, long long nA, long long nB, BankStepArgs args, float b1, float b2,
                                                                  float eps, float wd, float* __restrict__ norms) {
  __shared__ float red[16];
  __shared__ float s_coef;
  const int slot = blockIdx.x;
  const BankStepRec rc = args.rec[slot];
  if (!rc.active) { if (threadIdx.x == 0) norms[slot] = 0.f; return; }   // (uniform per workgroup) nothing of this slot is read or written
  float acc = 0.f;
  for (int part = 0; part < 2; ++part) {
    const float* g = part == 0 ? gA + slot * nA : gB + slot * nB;
    const long long n = part == 0 ? nA : nB;
    for (long long i = threadIdx.x; i < n; i += 1024) acc = fmaf(g[i], g[i], acc);
  }
  // fixed tree: lanes of a wave by shuffles, the 16 waves through LDS in wave order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float ss = 0.f;
    for (int k = 0; k < 16; ++k) ss += red[k];
    const float norm = sqrtf(ss);
    norms[slot] = norm;
    float c = 1.f;
    if (rc.max_norm > 0.f) { c = rc.max_norm / (norm + 1e-6f); c = c < 1.f ? c : 1.f; }
    s_coef = c;
  }
  __syncthreads();
  const float coef = s_coef, decay = 1.f - rc.lr * wd;
  for (int part = 0; part < 2; ++part) {
    const long long n = part == 0 ? nA : nB, off = slot * n;
    float* p = (part == 0 ? A32 : B32) + off; float* g = (part == 0 ? gA : gB) + off;
    float* mm = (part == 0 ? mA : mB) + off; float* vv = (part == 0 ? vA : vB) + off;
    T* sh = part == 0 ? A : B;
    for (long long i = threadIdx.x; i < n; i += 1024) {
      const float gk = g[i] * coef;
      const float pk = p[i] * decay;
      const float m1 = b1 * mm[i] + (1.f - b1) * gk;
      const float v1 = b2 * vv[i] + (1.f - b2) * gk * gk;
      const float denom = sqrtf(v1) / rc.bc2_sqrt + eps;
      const float pn = pk - (rc.lr / rc.bc1) * (m1 / denom);
      p[i] = pn; mm[i] = m1; vv[i] = v1; g[i] = 0.f;
      if (sh != nullptr) sh[off + i] = from_f32<T>(pn);
    }
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

void adapter_bank_free(Model* m) {
  if (m->bank) { (void)hipFree(m->bank->segA); (void)hipFree(m->bank->segB); }   // (grown on demand, so not in m->allocs)
  delete m->bank; m->bank = nullptr;
}

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
  if (b->train) {   // the slot's optimizer state belongs to the adapter that leaves: the next one starts from zero moments and step 0
    for (float* p : {b->gA, b->mA, b->vA}) HIP_CHECK(hipMemset(p + slot * na, 0, (size_t)na * 4));
    for (float* p : {b->gB, b->mB, b->vB}) HIP_CHECK(hipMemset(p + slot * nb, 0, (size_t)nb * 4));
    b->step[slot] = 0;
  }
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

// ------------------------------------------------------------------ the calls' side
// one entry of a caller's slot list `what`: -1 (the base model), or a slot that is complete
static int bank_entry_check(const Model* m, const char* what, int s) {
  ARG_CHECK(s >= -1 && s < RSYS_ADAPTER_SLOTS, std::string(what) + " entries must be in [-1, RSYS_ADAPTER_SLOTS)");
  if (s >= 0) ARG_CHECK(bank_complete(m, s), std::string(what) + " names a slot that is not complete (4 tensors per layer since its last clear)");
  return RSYS_OK;
}

// The buffers the bank allocates at their first use: La of the serving forward, and the tables of the packed calls (the tile maps in
// the caller's geometry, the segment table).  dalloc's zero fill runs on the null stream and the model's stream does not wait for that
// one, so a fresh fill is waited for HERE, before the caller queues anything on the model's stream: without that the fill may land on a
// table copied in behind it (every tile then reads slot 0 in the first packed call of a model), or on the first La.
enum { BANK_BUF_LA = 1, BANK_BUF_TILES = 2, BANK_BUF_PACK = 4 };
static int bank_first_use(Model* m, int which) {
  AdapterBank* b = m->bank;
  const int64_t tiles = (int64_t)m->rows_max * ((m->Sa + 31) / 32);
  bool fresh = false;
  auto once = [&](auto*& p, int64_t bytes) -> int {
    if (p) return RSYS_OK;
    fresh = true;
    DALLOC(p, bytes);
    return RSYS_OK;
  };
  HIP_CHECK(hipSetDevice(m->device));
  if (which & BANK_BUF_LA) RC(once(b->La, (int64_t)m->rows_max * m->Ta * 16 * m->esz));
  if (which & BANK_BUF_TILES) RC(once(b->d_tiles, tiles * 4));
  if (which & BANK_BUF_PACK) { RC(once(b->d_tile_task, tiles * 4)); RC(once(b->d_segs, tiles * 5 * 4)); }
  if (fresh) HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

// checks row_adapter[0 .. rows) and makes it the slot vector of the next forward_trunk (m->bank_rows); adapter_unbind_rows ends that
int adapter_bind_rows(Model* m, const int32_t* row_adapter) {
  RC(bank_check_model(m));
  ARG_CHECK(row_adapter != nullptr, "row_adapter is null (use rsys_infer_select for the base model)");
  ARG_CHECK(m->cur_rows > 0, "no batch uploaded");
  bool any = false;
  for (int r = 0; r < m->cur_rows; ++r) {
    RC(bank_entry_check(m, "row_adapter", row_adapter[r]));
    any |= row_adapter[r] >= 0;
  }
  m->bank_rows = nullptr;
  if (!any) return RSYS_OK;   // every row runs the base model: the forward launches what rsys_infer_select launches
  AdapterBank* b = m->bank;
  RC(bank_first_use(m, BANK_BUF_LA));
  HIP_CHECK(hipMemcpyAsync(b->d_rows, row_adapter, (size_t)m->cur_rows * 4, hipMemcpyHostToDevice, m->stream));
  m->bank_rows = b->d_rows;
  return RSYS_OK;
}
void adapter_unbind_rows(Model* m) { m->bank_rows = nullptr; m->bank_tiles = nullptr; }

// Packed serving rows: tile_adapter [rows][ceil(Sa / 32)] in the caller's geometry, entry j of row r = the slot of
// interactions [32 j, 32 j + 32) = tokens [64 j, 64 j + 64).  Every entry is checked; the ceil(S / 32) leading entries of each row -- the
// tiles the resident (possibly trimmed) rows have -- become the tile map of the next forward_trunk (m->bank_tiles).
int adapter_bind_tiles(Model* m, const int32_t* tile_adapter) {
  RC(bank_check_model(m));
  ARG_CHECK(tile_adapter != nullptr, "tile_adapter is null");
  ARG_CHECK(m->cur_rows > 0, "no batch uploaded");
  const int nta = (m->Sa + 31) / 32, nt = (m->S + 31) / 32;
  bool any = false;
  for (int i = 0; i < m->cur_rows * nta; ++i) {
    RC(bank_entry_check(m, "tile_adapter", tile_adapter[i]));
    any |= tile_adapter[i] >= 0 && i % nta < nt;
  }
  m->bank_rows = nullptr; m->bank_tiles = nullptr;
  if (!any) return RSYS_OK;   // every live tile runs the base model: the forward launches what rsys_infer_select launches
  AdapterBank* b = m->bank;
  RC(bank_first_use(m, BANK_BUF_LA | BANK_BUF_TILES));
  HIP_CHECK(hipStreamSynchronize(m->stream));   // (the previous call's copy has read h_tiles)
  b->h_tiles.resize((size_t)m->cur_rows * nt);
  for (int r = 0; r < m->cur_rows; ++r) std::copy(tile_adapter + (size_t)r * nta, tile_adapter + (size_t)r * nta + nt, b->h_tiles.begin() + (size_t)r * nt);
  HIP_CHECK(hipMemcpyAsync(b->d_tiles, b->h_tiles.data(), b->h_tiles.size() * 4, hipMemcpyHostToDevice, m->stream));
  m->bank_tiles = b->d_tiles;
  return RSYS_OK;
}

// One layer's launches on plain arguments: what the model-side callers below fill from Model and the test hooks (rsys_op_adapter_bank,
// rsys_debug.h) fill from the caller's buffers.  bankA / bankB: the compute-type copies; (p, seed, stream): the dropout key of BankDrop.
// The tile map, when set, takes the place of the row slots (packed rows: adapter_bind_tiles, rsys_adapter_forward_backward_packed, the
// _tiles / _segments hooks); the segment table comes with it in a training pass.
static BankLookup bank_lookup(const BankLaunch& a) {
  return a.tile_slot ? BankLookup{a.tile_slot, (a.Ttok + 63) / 64, a.segs} : BankLookup{a.row_slot, 0, nullptr};
}
template <typename T>
int bank_launch_a(const BankLaunch& a, const T* xn, T* La, bool train) {
  const dim3 grid((a.Ttok + BANK_A_TOK - 1) / BANK_A_TOK, a.rows);
  auto* kernel = train ? adapter_bank_a_kernel<T, true> : adapter_bank_a_kernel<T, false>;   // (train: the LoRA input under the dropout mask)
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, a.s, xn, (const T*)a.bankA, bank_lookup(a), a.layer, a.L, a.D, a.Ttok, La, a.p, a.seed, a.stream);
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}
template <typename T>
int bank_launch_b(const BankLaunch& a, const T* La, T* qkv, const float* rope_cos, const float* rope_sin, const int* rope_pos) {
  const int Nq = a.H * a.hd, Nk = a.KV * a.hd;
  const dim3 grid((a.Ttok + BANK_B_TOK - 1) / BANK_B_TOK, a.rows);
  hipLaunchKernelGGL((adapter_bank_b_kernel<T>), grid, dim3(256), 0, a.s, La, (const T*)a.bankB, bank_lookup(a), a.layer, a.L, Nq, Nk, Nk, a.Ttok, a.hd,
                     rope_cos, rope_sin, rope_pos, qkv);
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}
// the backward's launches in the order adapter_bank_backward issues them; `stages` as rsys_op_adapter_bank's mask (4 dLa, 8 dB partials,
// 16 dA partials, 32 dx, 64 both reductions).  partA / partB hold one partial per unit: [rows][..], or [n_seg][..] with a segment table.
template <typename T>
int bank_launch_backward(const BankLaunch& a, int stages, const T* xn, const T* dqkv, const T* La, T* dLa, T* dxn, float* partA, float* partB,
                         float* gA, float* gB) {
  const int rows = a.rows, Nq = a.H * a.hd, Nk = a.KV * a.hd, Nv = Nk, Ttok = a.Ttok, D = a.D;
  const BankLookup look = bank_lookup(a);
  const int units = look.segs ? a.n_seg : rows;
  hipStream_t s = a.s;
  if (stages & 4)
    hipLaunchKernelGGL((adapter_bank_dla_kernel<T>), dim3((Ttok + BANK_A_TOK - 1) / BANK_A_TOK, rows), dim3(256), 0, s, dqkv, (const T*)a.bankB, look,
                       a.layer, a.L, Nq, Nk, Nv, Ttok, dLa);
  if (stages & 8)
    hipLaunchKernelGGL((adapter_bank_db_kernel<T>), dim3((Nq + Nv + 63) / 64, units), dim3(256), 0, s, dqkv, La, look, Nq, Nk, Nv, Ttok, partB);
  if (stages & 16)
    hipLaunchKernelGGL((adapter_bank_da_kernel<T>), dim3((D + 63) / 64, units), dim3(256), 0, s, (const T*)dLa, xn, look, D, Ttok, partA, a.p, a.seed,
                       a.stream);
  if (stages & 32)
    hipLaunchKernelGGL((adapter_bank_dx_kernel<T>), dim3((Ttok + BANK_B_TOK - 1) / BANK_B_TOK, rows), dim3(256), 0, s, (const T*)dLa, (const T*)a.bankA,
                       look, a.layer, a.L, D, Ttok, dxn, a.p, a.seed, a.stream);
  if (stages & 64) {
    const long long na = (long long)16 * D, nb = (long long)(Nq + Nv) * 8;
    const int* key = look.segs ? look.segs + 3 : look.map;
    auto* reduce = look.segs ? adapter_bank_reduce_kernel<5> : adapter_bank_reduce_kernel<1>;
    hipLaunchKernelGGL(reduce, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, s, partA, key, units, na, 1.f, gA + (long long)a.layer * na,
                       (long long)a.L * na);
    hipLaunchKernelGGL(reduce, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, partB, key, units, nb, 2.f, gB + (long long)a.layer * nb,
                       (long long)a.L * nb);
  }
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}

static BankLaunch bank_launch_of(const Model* m, int l) {
  const AdapterBank* b = m->bank;
  BankLaunch a{};
  a.rows = m->cur_rows; a.Ttok = m->T; a.D = m->D; a.H = m->H; a.KV = m->KV; a.hd = m->hd; a.L = m->L; a.layer = l;
  a.row_slot = m->bank_rows; a.tile_slot = m->bank_tiles; a.bankA = b->A; a.bankB = b->B;
  if (m->bank_packed) { a.segs = b->d_segs; a.n_seg = b->n_seg; }
  a.p = b->drop_now ? b->dropout : 0.f; a.seed = m->drop_seed; a.stream = (unsigned int)(m->drop_step * 64 + l);
  a.s = m->stream;
  return a;
}

template <typename T>
int adapter_bank_stage_a(Model* m, int l, const T* xn) {
  const AdapterBank* b = m->bank;
  tic(m, "hbm_adapter_bank_a", (double)sizeof(T) * m->cur_rows * m->T * (m->D + 16.0));
  // a training pass writes the layer's own La (the backward reads it)
  RC(bank_launch_a<T>(bank_launch_of(m, l), xn, m->bank_train ? bank_la<T>(m, l) : (T*)b->La, m->bank_train));
  toc(m);
  return RSYS_OK;
}
template <typename T>
int adapter_bank_stage_b(Model* m, int l, T* qkv, const int* rope_pos) {
  const AdapterBank* b = m->bank;
  const int rows = m->cur_rows, Nq = m->H * m->hd, Nk = m->KV * m->hd;
  tic(m, "hbm_adapter_bank_b", (double)sizeof(T) * rows * m->T * (2.0 * (Nq + Nk) + 16.0));
  RC(bank_launch_b<T>(bank_launch_of(m, l), m->bank_train ? (const T*)bank_la<T>(m, l) : (const T*)b->La, qkv, m->rope_cos, m->rope_sin, rope_pos));
  toc(m);
  return RSYS_OK;
}
template int adapter_bank_stage_a<float>(Model*, int, const float*);
template int adapter_bank_stage_a<bf16>(Model*, int, const bf16*);
template int adapter_bank_stage_b<float>(Model*, int, float*, const int*);
template int adapter_bank_stage_b<bf16>(Model*, int, bf16*, const int*);

// ------------------------------------------------------------------ training through the bank: host side
static int bank_train_check_model(const Model* m) {
  RC(bank_check_model(m));
  ARG_CHECK(!m->sharded, "adapter bank training: a model with a replicated item table");
  return RSYS_OK;
}

int adapter_train_enable(Model* m, float dropout) {
  RC(bank_train_check_model(m));
  ARG_CHECK(dropout >= 0.f && dropout < 1.f, "adapter bank training: dropout must be in [0, 1)");
  ARG_CHECK(m->Ta % 8 == 0 && m->D % 16 == 0 && m->hd % 8 == 0, "adapter bank training: 2 S % 8, embed_dim % 16 and head_dim % 8 must be 0");
  RC(bank_ensure(m));
  AdapterBank* b = m->bank;
  HIP_CHECK(hipSetDevice(m->device));
  if (!b->train) {
    const int64_t na = (int64_t)RSYS_ADAPTER_SLOTS * m->L * bank_a_floats(m), nb = (int64_t)RSYS_ADAPTER_SLOTS * m->L * bank_b_floats(m);
    const int64_t tok = (int64_t)m->rows_max * m->Ta;
    // (every buffer once: a call that failed part-way is taken up where it stopped)
#define BANK_ONCE(ptr, bytes) do { if ((ptr) == nullptr) DALLOC(ptr, bytes); } while (0)
    BANK_ONCE(b->gA, na * 4); BANK_ONCE(b->gB, nb * 4);
    BANK_ONCE(b->mA, na * 4); BANK_ONCE(b->vA, na * 4); BANK_ONCE(b->mB, nb * 4); BANK_ONCE(b->vB, nb * 4);
    BANK_ONCE(b->La_l, (int64_t)m->L * tok * 16 * m->esz); BANK_ONCE(b->dLa, tok * 16 * m->esz);
    BANK_ONCE(b->partA, (int64_t)m->rows_max * bank_a_floats(m) * 4); BANK_ONCE(b->partB, (int64_t)m->rows_max * bank_b_floats(m) * 4);
    BANK_ONCE(b->d_task, (int64_t)m->rows_max * 4); BANK_ONCE(b->d_norms, RSYS_ADAPTER_SLOTS * 4);
    BANK_ONCE(m->bank_sink, (int64_t)std::max(m->D, 64) * 4);
#undef BANK_ONCE
    // the pass runs with every sum of the trunk in a fixed order too, whatever the model's own setting: it needs that mode's scratch
    RC(model_ensure_det_scratch(m));
    b->train = true;
  }
  b->dropout = dropout;
  return RSYS_OK;
}

// what both training calls require of the model and its resident batch
static int bank_train_call_check(Model* m) {
  RC(bank_train_check_model(m));
  ARG_CHECK(m->bank != nullptr && m->bank->train, "adapter bank training is not enabled (rsys_adapter_train_enable)");
  ARG_CHECK(m->cur_rows > 0, "no batch uploaded");
  return check_not_trimmed(m);
}

// One unit of a training call -- `unit` = "row" or "segment" -- names a slot and a task, or neither; and one task has one slot per call
// (owner[task], -1 while nobody named it).
static int bank_pair_check(const char* unit, int s, int t, int (&owner)[4]) {
  const std::string u(unit);
  ARG_CHECK(s >= -1 && s < RSYS_ADAPTER_SLOTS, u + " slots must be in [-1, RSYS_ADAPTER_SLOTS)");
  ARG_CHECK(t >= -1 && t < 4, u + " tasks must be in [-1, 4)");
  ARG_CHECK((s < 0) == (t < 0), "a " + u + " names a slot and a task, or neither (-1 / -1)");
  if (s < 0) return RSYS_OK;
  ARG_CHECK(owner[t] < 0 || owner[t] == s, "one task is named by two slots in the same call");
  owner[t] = s;
  return RSYS_OK;
}

// One training pass over the resident batch with the tables the caller has queued on the model's stream: the slot per row or (packed)
// per tile -- nullptr when every unit runs the base model -- and the task per row or tile.  The pass runs with every sum in a fixed
// order whatever the model's own setting; what it sets is put back on every return path.
static int bank_train_pass(Model* m, int evaluate, const int* rows, const int* tiles, bool packed, const int* d_task, float grad_scale, uint64_t seed,
                           uint64_t step) {
  AdapterBank* b = m->bank;
  const bool det = m->deterministic;
  m->deterministic = true;
  m->bank_rows = rows; m->bank_tiles = tiles;
  m->bank_train = true;
  m->bank_packed = packed;   // masks per tile; the last layer runs dense (its compact order would mix segments inside a work item)
  b->drop_now = !evaluate && b->dropout > 0.f;
  int rc;
  {
    DetScope scope(m);
    rc = model_forward_backward_rows(m, evaluate, d_task, grad_scale, seed, step);
  }
  m->bank_packed = false;
  m->bank_train = false;
  m->bank_rows = nullptr; m->bank_tiles = nullptr;
  m->deterministic = det;
  return rc;
}

int adapter_forward_backward(Model* m, int evaluate, const int32_t* row_slot, const int32_t* row_task, float grad_scale, uint64_t seed, uint64_t step) {
  RC(bank_train_call_check(m));
  ARG_CHECK(row_slot != nullptr && row_task != nullptr, "row_slot / row_task is null");
  int owner[4] = {-1, -1, -1, -1};
  bool any = false;
  for (int r = 0; r < m->cur_rows; ++r) {
    RC(bank_pair_check("row", row_slot[r], row_task[r], owner));
    RC(bank_entry_check(m, "row_slot", row_slot[r]));
    any |= row_slot[r] >= 0;
  }
  AdapterBank* b = m->bank;
  HIP_CHECK(hipSetDevice(m->device));
  HIP_CHECK(hipMemcpyAsync(b->d_rows, row_slot, (size_t)m->cur_rows * 4, hipMemcpyHostToDevice, m->stream));
  HIP_CHECK(hipMemcpyAsync(b->d_task, row_task, (size_t)m->cur_rows * 4, hipMemcpyHostToDevice, m->stream));
  return bank_train_pass(m, evaluate, any ? b->d_rows : nullptr, nullptr, false, b->d_task, grad_scale, seed, step);
}

// The segment table of a packed call, checked on the host (rsys_adapter_forward_backward_packed and rsys_op_adapter_bank_segments): seg
// [n_seg][5] = (row, first column, columns, slot, task) on rows of S interactions.  Fills the [rows][ceil(S / 32)] tile maps of slot and task
// (-1 where no segment, or a base-model segment, lies) and says whether any segment names a slot.
static int bank_segs_check(const int32_t* seg, int n_seg, int rows, int S, std::vector<int32_t>* tile_slot, std::vector<int32_t>* tile_task, bool* any) {
  TileOwners tiles(rows, S);
  ARG_CHECK(seg != nullptr, "segment table is null");
  ARG_CHECK(n_seg >= 1 && (long long)n_seg <= (long long)rows * tiles.nt && n_seg <= 65535, "n_seg must be in [1, rows * ceil(S / 32)]");
  int owner[4] = {-1, -1, -1, -1};
  *any = false;
  for (int i = 0; i < n_seg; ++i) {
    const int32_t* g = seg + (size_t)i * 5;
    ARG_CHECK(g[2] >= 1, "a segment lies inside its row, on at least one column");
    RC(tiles.place("adapter bank", g[0], g[1], g[2], i));
    RC(bank_pair_check("segment", g[3], g[4], owner));
    *any |= g[3] >= 0;
  }
  tile_slot->assign(tiles.owner.size(), -1); tile_task->assign(tiles.owner.size(), -1);
  for (size_t k = 0; k < tiles.owner.size(); ++k)
    if (tiles.owner[k] >= 0) { (*tile_slot)[k] = seg[(size_t)tiles.owner[k] * 5 + 3]; (*tile_task)[k] = seg[(size_t)tiles.owner[k] * 5 + 4]; }
  return RSYS_OK;
}

// rsys_adapter_forward_backward on packed rows: several users per row, each in a segment of whole 64-token tiles that names
// its slot and task.  The caller guarantees the resident columns (one non-zero userid per segment, distinct within a row, zeros elsewhere).
int adapter_forward_backward_packed(Model* m, int evaluate, const int32_t* seg, int n_seg, float grad_scale, uint64_t seed, uint64_t step) {
  RC(bank_train_call_check(m));
  std::vector<int32_t> ts, tt;
  bool any = false;
  RC(bank_segs_check(seg, n_seg, m->cur_rows, m->S, &ts, &tt, &any));
  for (int i = 0; i < n_seg; ++i) RC(bank_entry_check(m, "the segment table", seg[(size_t)i * 5 + 3]));
  AdapterBank* b = m->bank;
  RC(bank_first_use(m, BANK_BUF_TILES | BANK_BUF_PACK));   // (full rows: the caller's geometry is the resident one)
  HIP_CHECK(hipStreamSynchronize(m->stream));   // (the previous call's copies have read h_pack, its kernels the partials)
  if (n_seg > b->seg_cap) {
    float *na = nullptr, *nb = nullptr;
    HIP_CHECK(hipMalloc((void**)&na, (size_t)n_seg * bank_a_floats(m) * 4));
    if (hipMalloc((void**)&nb, (size_t)n_seg * bank_b_floats(m) * 4) != hipSuccess) { (void)hipFree(na); set_error("adapter bank: out of device memory for the segment partials"); return RSYS_ERR_HIP; }
    (void)hipFree(b->segA); (void)hipFree(b->segB);
    b->segA = na; b->segB = nb; b->seg_cap = n_seg;
  }
  const size_t ntile = ts.size();
  b->h_pack.resize(2 * ntile + (size_t)n_seg * 5);
  std::copy(ts.begin(), ts.end(), b->h_pack.begin());
  std::copy(tt.begin(), tt.end(), b->h_pack.begin() + ntile);
  std::copy(seg, seg + (size_t)n_seg * 5, b->h_pack.begin() + 2 * ntile);
  HIP_CHECK(hipMemcpyAsync(b->d_tiles, b->h_pack.data(), ntile * 4, hipMemcpyHostToDevice, m->stream));
  HIP_CHECK(hipMemcpyAsync(b->d_tile_task, b->h_pack.data() + ntile, ntile * 4, hipMemcpyHostToDevice, m->stream));
  HIP_CHECK(hipMemcpyAsync(b->d_segs, b->h_pack.data() + 2 * ntile, (size_t)n_seg * 5 * 4, hipMemcpyHostToDevice, m->stream));
  b->n_seg = n_seg;
  return bank_train_pass(m, evaluate, nullptr, any ? b->d_tiles : nullptr, true, b->d_tile_task, grad_scale, seed, step);
}

template <typename T>
int adapter_bank_backward(Model* m, int l, const T* xn, const T* dqkv, T* dxn) {
  if (!m->bank_rows && !m->bank_tiles) return RSYS_OK;   // every row runs the base model: nothing to differentiate
  AdapterBank* b = m->bank;
  tic(m, "adapter_bank_bwd");
  RC(bank_launch_backward<T>(bank_launch_of(m, l), 4 | 8 | 16 | 32 | 64, xn, dqkv, (const T*)bank_la<T>(m, l), (T*)b->dLa, dxn,
                             m->bank_packed ? b->segA : b->partA, m->bank_packed ? b->segB : b->partB, b->gA, b->gB));
  toc(m);
  return RSYS_OK;
}
template int adapter_bank_backward<float>(Model*, int, const float*, const float*, float*);
template int adapter_bank_backward<bf16>(Model*, int, const bf16*, const bf16*, bf16*);

// rsys_op_adapter_bank (rsys_debug.h): the launches above on the caller's device buffers, in production order, then a device synchronise.
// Every refusal comes before the first launch.
template <typename T>
static int bank_op_run(const BankLaunch& a, int stages, int train, const void* xn, void* La, void* qkv, const void* dqkv, void* dLa, void* dxn,
                       float* partA, float* partB, float* gA, float* gB, const float* rope_cos, const float* rope_sin, const int* rope_pos) {
  if (stages & 1) RC(bank_launch_a<T>(a, (const T*)xn, (T*)La, train != 0));
  if (stages & 2) RC(bank_launch_b<T>(a, (const T*)La, (T*)qkv, rope_cos, rope_sin, rope_pos));
  if (stages & 124) RC(bank_launch_backward<T>(a, stages, (const T*)xn, (const T*)dqkv, (const T*)La, (T*)dLa, (T*)dxn, partA, partB, gA, gB));
  return RSYS_OK;
}
int adapter_bank_op(int dtype, int stages, int train, int rows, int Ttok, int D, int H, int KV, int hd, int L, int layer, float p, uint64_t seed,
                    int64_t stream, const int32_t* row_slot, const void* bankA, const void* bankB, const void* xn, void* La, void* qkv, const void* dqkv,
                    void* dLa, void* dxn, float* partA, float* partB, float* gA, float* gB, const float* rope_cos, const float* rope_sin,
                    const int32_t* rope_pos, int rope_rows, int tiles, int n_seg) {
  // (tiles == 1, rsys_op_adapter_bank_tiles: row_slot is the tile map [rows][ceil(Ttok / 64)] and the two forward stages take their slot per tile;
  //  tiles == 2, rsys_op_adapter_bank_segments: row_slot is the segment table [n_seg][5], the token stages take their slot per tile, the partials and sums their range per segment)
  ARG_CHECK(tiles != 1 || ((stages & ~3) == 0 && train == 0), "rsys_op_adapter_bank_tiles: stages 1 and 2 only (the forward, train = 0)");
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_adapter_bank: dtype fp32 or bf16");
  ARG_CHECK(stages >= 1 && stages <= 127, "rsys_op_adapter_bank: stages is a mask of bits 1 .. 64");
  ARG_CHECK(rows >= 1 && rows <= 65535 && Ttok >= 8 && L >= 1 && layer >= 0 && layer < L && H >= 1 && KV >= 1, "rsys_op_adapter_bank: empty shape or layer outside [0, L)");
  ARG_CHECK(Ttok % 8 == 0, "rsys_op_adapter_bank: Ttok % 8 must be 0");
  ARG_CHECK(D >= 16 && D % 16 == 0, "rsys_op_adapter_bank: D % 16 must be 0");
  ARG_CHECK(hd == 16 || hd == 32 || hd == 64 || hd == 128, "rsys_op_adapter_bank: hd must be 16, 32, 64 or 128");
  ARG_CHECK(D == H * hd, "rsys_op_adapter_bank: D must be H * hd");
  ARG_CHECK(H % KV == 0, "rsys_op_adapter_bank: H % KV must be 0");
  ARG_CHECK(p >= 0.f && p < 1.f, "rsys_op_adapter_bank: dropout p must be in [0, 1)");
  ARG_CHECK(stream >= 0 && stream <= 0xFFFFFFFFLL, "rsys_op_adapter_bank: stream is a 32-bit counter word");
  ARG_CHECK(row_slot != nullptr, "rsys_op_adapter_bank: row_slot is null");
  ARG_CHECK(!(stages & (1 | 32)) || bankA, "rsys_op_adapter_bank: stage A and dx read bankA");
  ARG_CHECK(!(stages & (2 | 4)) || bankB, "rsys_op_adapter_bank: stage B and dLa read bankB");
  ARG_CHECK(!(stages & (1 | 16)) || xn, "rsys_op_adapter_bank: stage A and dA read xn");
  ARG_CHECK(!(stages & (1 | 2 | 8)) || La, "rsys_op_adapter_bank: stage A, stage B and dB use La");
  ARG_CHECK(!(stages & 2) || (qkv && rope_cos && rope_sin), "rsys_op_adapter_bank: stage B needs qkv and the rope tables");
  ARG_CHECK(!(stages & (4 | 8)) || dqkv, "rsys_op_adapter_bank: dLa and dB read dqkv");
  ARG_CHECK(!(stages & (4 | 16 | 32)) || dLa, "rsys_op_adapter_bank: dLa, dA and dx use dLa");
  ARG_CHECK(!(stages & 32) || dxn, "rsys_op_adapter_bank: dx needs dxn");
  ARG_CHECK(!(stages & (16 | 64)) || partA, "rsys_op_adapter_bank: dA and the reductions use partA");
  ARG_CHECK(!(stages & (8 | 64)) || partB, "rsys_op_adapter_bank: dB and the reductions use partB");
  ARG_CHECK(!(stages & 64) || (gA && gB), "rsys_op_adapter_bank: the reductions need gA and gB");
  std::vector<int32_t> host((size_t)rows * (tiles ? (Ttok + 63) / 64 : 1)), seg_tiles, seg_tasks;
  if (tiles == 2) {   // the segment table, checked as rsys_adapter_forward_backward_packed checks it (rows of Ttok / 2 interactions)
    ARG_CHECK(n_seg >= 1 && n_seg <= 65535, "rsys_op_adapter_bank_segments: n_seg must be in [1, rows * ceil(Ttok / 64)]");
    host.resize((size_t)n_seg * 5);
    HIP_CHECK(hipMemcpy(host.data(), row_slot, host.size() * 4, hipMemcpyDeviceToHost));
    bool any = false;
    RC(bank_segs_check(host.data(), n_seg, rows, Ttok / 2, &seg_tiles, &seg_tasks, &any));
  } else {
    HIP_CHECK(hipMemcpy(host.data(), row_slot, host.size() * 4, hipMemcpyDeviceToHost));
    for (int32_t v : host) ARG_CHECK(v >= -1 && v < RSYS_ADAPTER_SLOTS, "rsys_op_adapter_bank: row_slot entries must be in [-1, RSYS_ADAPTER_SLOTS)");
  }
  if ((stages & 2) && rope_pos) {   // every explicit position inside the tables (one copy back)
    host.resize((size_t)rows * Ttok);
    HIP_CHECK(hipMemcpy(host.data(), rope_pos, host.size() * 4, hipMemcpyDeviceToHost));
    for (int32_t v : host) ARG_CHECK(v >= 0 && v < rope_rows, "rsys_op_adapter_bank: rope_pos outside the tables");
  } else if (stages & 2) {
    ARG_CHECK(rope_rows >= Ttok, "rsys_op_adapter_bank: rope tables shorter than Ttok");
  }
  BankLaunch a{};
  a.rows = rows; a.Ttok = Ttok; a.D = D; a.H = H; a.KV = KV; a.hd = hd; a.L = L; a.layer = layer;
  int* d_seg_tiles = nullptr;
  if (tiles == 2) {   // (partA / partB: [n_seg][16][D], [n_seg][Nq + Nv][8])
    HIP_CHECK(hipMalloc((void**)&d_seg_tiles, seg_tiles.size() * 4));
    if (hipMemcpy(d_seg_tiles, seg_tiles.data(), seg_tiles.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d_seg_tiles); set_error("rsys_op_adapter_bank_segments: tile map upload failed"); return RSYS_ERR_HIP; }
    a.segs = row_slot; a.n_seg = n_seg;
  }
  a.row_slot = tiles ? nullptr : row_slot; a.tile_slot = tiles == 2 ? d_seg_tiles : tiles ? row_slot : nullptr; a.bankA = bankA; a.bankB = bankB; a.p = p; a.seed = seed; a.stream = (unsigned int)stream; a.s = nullptr;
  int rc = dtype == RSYS_DTYPE_BF16
               ? bank_op_run<bf16>(a, stages, train, xn, La, qkv, dqkv, dLa, dxn, partA, partB, gA, gB, rope_cos, rope_sin, rope_pos)
               : bank_op_run<float>(a, stages, train, xn, La, qkv, dqkv, dLa, dxn, partA, partB, gA, gB, rope_cos, rope_sin, rope_pos);
  hipError_t e = hipDeviceSynchronize();
  if (d_seg_tiles) (void)hipFree(d_seg_tiles);
  if (rc) return rc;
  HIP_CHECK(e);
  return RSYS_OK;
}

// a slot's tensor in one of the training buffers (which: 0 gradient, 1 exp_avg, 2 exp_avg_sq)
static int bank_train_locate(Model* m, int slot, const char* name, int64_t n, float** g, float** mo, float** va) {
  RC(bank_train_check_model(m));
  ARG_CHECK(m->bank != nullptr && m->bank->train, "adapter bank training is not enabled (rsys_adapter_train_enable)");
  ARG_CHECK(slot >= 0 && slot < RSYS_ADAPTER_SLOTS, "adapter slot must be in [0, RSYS_ADAPTER_SLOTS)");
  int layer, which;
  if (!bank_parse_name(m, name, &layer, &which)) { set_error(std::string("unknown adapter tensor: ") + name); return RSYS_ERR_ARG; }
  bool in_b; int64_t off, cnt;
  bank_locate(m, slot, layer, which, &in_b, &off, &cnt);
  ARG_CHECK(n == cnt, "element count does not match the adapter tensor's shape");
  AdapterBank* b = m->bank;
  *g = (in_b ? b->gB : b->gA) + off; *mo = (in_b ? b->mB : b->mA) + off; *va = (in_b ? b->vB : b->vA) + off;
  return RSYS_OK;
}

int adapter_grad_get(Model* m, int slot, const char* name, float* out, int64_t n) {
  ARG_CHECK(name != nullptr && out != nullptr, "null");
  float *g, *mo, *va;
  RC(bank_train_locate(m, slot, name, n, &g, &mo, &va));
  HIP_CHECK(hipSetDevice(m->device));
  HIP_CHECK(hipStreamSynchronize(m->stream));
  HIP_CHECK(hipMemcpy(out, g, (size_t)n * 4, hipMemcpyDeviceToHost));
  return RSYS_OK;
}

int adapter_zero_grad(Model* m) {
  RC(bank_train_check_model(m));
  ARG_CHECK(m->bank != nullptr && m->bank->train, "adapter bank training is not enabled (rsys_adapter_train_enable)");
  AdapterBank* b = m->bank;
  HIP_CHECK(hipSetDevice(m->device));
  HIP_CHECK(hipMemsetAsync(b->gA, 0, (size_t)RSYS_ADAPTER_SLOTS * m->L * bank_a_floats(m) * 4, m->stream));
  HIP_CHECK(hipMemsetAsync(b->gB, 0, (size_t)RSYS_ADAPTER_SLOTS * m->L * bank_b_floats(m) * 4, m->stream));
  return RSYS_OK;
}

// one slot's record of the optimizer launch: the bias corrections of step `t` (1-based) in the host arithmetic every caller shares
static BankStepRec bank_step_rec(bool active, float lr, float max_norm, int t, float b1, float b2) {
  BankStepRec r{};
  r.active = active ? 1 : 0;
  if (!active) return r;
  const float tf = (float)t;
  r.lr = lr; r.max_norm = max_norm;
  r.bc1 = 1.f - powf(b1, tf); r.bc2_sqrt = sqrtf(1.f - powf(b2, tf));
  return r;
}
// the optimizer launch on plain arguments (A / B: the compute-type copies, used in bf16 mode only)
static int bank_launch_adamw(bool bf16_mode, int n_slots, float* A32, float* B32, float* gA, float* gB, float* mA, float* vA, float* mB, float* vB, void* A,
                             void* B, long long na, long long nb, const BankStepArgs& a, float b1, float b2, float eps, float wd, float* norms,
                             hipStream_t s) {
  if (bf16_mode)
    hipLaunchKernelGGL((adapter_bank_adamw_kernel<bf16>), dim3(n_slots), dim3(1024), 0, s, A32, B32, gA, gB, mA, vA, mB, vB, (bf16*)A, (bf16*)B, na, nb, a, b1,
                       b2, eps, wd, norms);
  else
    hipLaunchKernelGGL((adapter_bank_adamw_kernel<float>), dim3(n_slots), dim3(1024), 0, s, A32, B32, gA, gB, mA, vA, mB, vB, (float*)nullptr,
                       (float*)nullptr, na, nb, a, b1, b2, eps, wd, norms);
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}

int adapter_adamw_step(Model* m, float lr0, float b1, float b2, float eps, float wd, const float* per_slot, int n_slots, float* norms_out) {
  RC(bank_train_check_model(m));
  ARG_CHECK(m->bank != nullptr && m->bank->train, "adapter bank training is not enabled (rsys_adapter_train_enable)");
  ARG_CHECK(per_slot != nullptr && norms_out != nullptr, "per_slot / norms_out is null");
  ARG_CHECK(n_slots >= 1 && n_slots <= RSYS_ADAPTER_SLOTS, "n_slots must be in [1, RSYS_ADAPTER_SLOTS]");
  for (int s = 0; s < n_slots; ++s)
    if (per_slot[3 * s] != 0.f) ARG_CHECK(bank_complete(m, s), "an active slot is not complete (4 tensors per layer since its last clear)");
  AdapterBank* b = m->bank;
  BankStepArgs a{};
  for (int s = 0; s < n_slots; ++s)   // (the count itself moves once the kernel is enqueued)
    a.rec[s] = bank_step_rec(per_slot[3 * s] != 0.f, lr0 * per_slot[3 * s + 1], per_slot[3 * s + 2], b->step[s] + 1, b1, b2);
  HIP_CHECK(hipSetDevice(m->device));
  const long long na = (long long)m->L * bank_a_floats(m), nb = (long long)m->L * bank_b_floats(m);
  RC(bank_launch_adamw(m->bf16_mode, n_slots, b->A32, b->B32, b->gA, b->gB, b->mA, b->vA, b->mB, b->vB, b->A, b->B, na, nb, a, b1, b2, eps, wd, b->d_norms,
                       m->stream));
  for (int s = 0; s < n_slots; ++s) b->step[s] += a.rec[s].active;
  HIP_CHECK(hipMemcpyAsync(norms_out, b->d_norms, (size_t)n_slots * 4, hipMemcpyDeviceToHost, m->stream));
  HIP_CHECK(hipStreamSynchronize(m->stream));
  return RSYS_OK;   // (no parameter of the trunk changed: table_dirty / wt_dirty stay as they are)
}

// rsys_op_adapter_bank_adamw (rsys_debug.h): per_slot [RSYS_ADAPTER_SLOTS][4] = (active, lr, max_norm, step), step = the 1-based count the
// bias corrections are taken at
int adapter_bank_adamw_op(int dtype, float* A32, float* B32, float* gA, float* gB, float* mA, float* vA, float* mB, float* vB, void* A, void* B,
                          int64_t nA, int64_t nB, const float* per_slot, float b1, float b2, float eps, float wd, float* norms) {
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_adapter_bank_adamw: dtype fp32 or bf16");
  ARG_CHECK(A32 && B32 && gA && gB && mA && vA && mB && vB && per_slot && norms && nA >= 1 && nB >= 1, "rsys_op_adapter_bank_adamw: null or empty");
  const bool bf = dtype == RSYS_DTYPE_BF16;
  ARG_CHECK(!bf || (A && B), "rsys_op_adapter_bank_adamw: bf16 needs the compute-type copies");
  BankStepArgs a{};
  for (int s = 0; s < RSYS_ADAPTER_SLOTS; ++s) {
    const float* q = per_slot + 4 * s;
    ARG_CHECK(q[0] == 0.f || q[3] >= 1.f, "rsys_op_adapter_bank_adamw: an active slot's step must be >= 1");
    a.rec[s] = bank_step_rec(q[0] != 0.f, q[1], q[2], (int)q[3], b1, b2);
  }
  int rc = bank_launch_adamw(bf, RSYS_ADAPTER_SLOTS, A32, B32, gA, gB, mA, vA, mB, vB, A, B, nA, nB, a, b1, b2, eps, wd, norms, nullptr);
  hipError_t e = hipDeviceSynchronize();
  if (rc) return rc;
  HIP_CHECK(e);
  return RSYS_OK;
}

int adapter_adamw_state_io(Model* m, int slot, const char* name, float* m_out, float* v_out, const float* m_in, const float* v_in, int64_t n,
                           int32_t* step_out, int32_t step_in) {
  RC(bank_train_check_model(m));
  ARG_CHECK(m->bank != nullptr && m->bank->train, "adapter bank training is not enabled (rsys_adapter_train_enable)");
  ARG_CHECK(slot >= 0 && slot < RSYS_ADAPTER_SLOTS, "adapter slot must be in [0, RSYS_ADAPTER_SLOTS)");
  AdapterBank* b = m->bank;
  if (name != nullptr) {
    const bool get = m_out != nullptr || v_out != nullptr;
    ARG_CHECK(get ? (m_out && v_out) : (m_in && v_in), "exp_avg and exp_avg_sq are both given");
    float *g, *mo, *va;
    RC(bank_train_locate(m, slot, name, n, &g, &mo, &va));
    HIP_CHECK(hipSetDevice(m->device));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    if (get) {
      HIP_CHECK(hipMemcpy(m_out, mo, (size_t)n * 4, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(v_out, va, (size_t)n * 4, hipMemcpyDeviceToHost));
    } else {
      HIP_CHECK(hipMemcpy(mo, m_in, (size_t)n * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(va, v_in, (size_t)n * 4, hipMemcpyHostToDevice));
    }
  }
  if (step_out) *step_out = b->step[slot];
  if (step_in >= 0) b->step[slot] = step_in;
  return RSYS_OK;
}

}  // namespace rsys
