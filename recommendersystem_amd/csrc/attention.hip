// Block-sparse bidirectional attention with the reference's two-predicate mask
// (transformer.model.py:479-487): allowed(q,kv) = userid[q]==userid[kv] AND
// (tmid[kv]==0 OR tmid[q]==tmid[kv]); GQA (q head h -> kv head h/(H/KV)); scores
// scaled by 1/sqrt(hd) (flex_attention default, model.py:278-285).
//
// gfx950 design.  64x64 (q x kv) tiles, 4 waves per workgroup, 16 q (or kv) per wave ON THE LANES:
// every first-stage product is computed transposed (S^T = K Q^T: rows = kv in the accumulator registers,
// column = q on the lane), so
//   * softmax statistics of a query are lane-local (16 values + two cross-group shuffles), and
//   * the probabilities never leave the registers: a 16x16 accumulator tile IS the B operand of the next
//     MFMA (cdna_hip_programming.md section 3, "An accumulator tile as the next MFMA's operand"); the
//     matching A operand (V^T, K^T, Q^T, dO^T fragments with the same k-slot order) is read from the
//     row-major LDS tile with ds_read_b64_tr_b16 -- no transposed copies in HBM, no P round trip through LDS.
// Tile pairs with no allowed element are skipped, pairs where every element is allowed skip the mask
// arithmetic (two bitmaps per row built once per step; the reference rebuilds a dense block mask every step,
// model.py:488-490).  K/V (resp. Q/dO) tiles are double-buffered in LDS, one barrier per tile.
// Backward is two kernels (dK/dV per kv tile, dQ per q tile): no float atomics, bitwise reproducible.
#include "kernels.hpp"

namespace rsys {

#define SENT_Q (-2147483647)
#define SENT_K (-2147483646)
// token keys (uid << 12 | tm) of tokens past the end of a row: never equal to each other or to a real key (uid < 2^19)
#define KEY_NO_Q ((int)0xFFFFE000u)
#define KEY_NO_K ((int)0xFFFFFFFFu)
constexpr float LOG2E = 1.4426950408889634f;
// v_exp_f32 directly (exp2f adds range scaling the softmax arguments never need: they are <= 0 or hugely negative)
__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

// max / sum over the four lanes that share a query (lane, lane ^ 16, lane ^ 32, lane ^ 48): two row swaps in the vector
// ALU (v_permlane16_swap / v_permlane32_swap) instead of two ds_bpermute round trips through the LDS pipeline, which put
// ~5 index instructions and an LDS latency each into the soft-max's dependency chain.
__device__ __forceinline__ float quad_rows_max(float v) {
  const unsigned int u = __builtin_bit_cast(unsigned int, v);
  auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  v = fmaxf(__builtin_bit_cast(float, (unsigned int)a[0]), __builtin_bit_cast(float, (unsigned int)a[1]));
  const unsigned int w = __builtin_bit_cast(unsigned int, v);
  auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return fmaxf(__builtin_bit_cast(float, (unsigned int)b[0]), __builtin_bit_cast(float, (unsigned int)b[1]));
}
__device__ __forceinline__ float quad_rows_sum(float v) {
  const unsigned int u = __builtin_bit_cast(unsigned int, v);
  auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  v = __builtin_bit_cast(float, (unsigned int)a[0]) + __builtin_bit_cast(float, (unsigned int)a[1]);
  const unsigned int w = __builtin_bit_cast(unsigned int, v);
  auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return __builtin_bit_cast(float, (unsigned int)b[0]) + __builtin_bit_cast(float, (unsigned int)b[1]);
}

template <typename T> struct AMma;
template <> struct AMma<bf16> {
  static constexpr int KS = 32;   // contraction per MFMA
  // (register-staged kernels; every head size: rows of 96 / 96 / 160 / 288 bytes for head_dim 16 / 32 / 64 / 128 are all free of conflicts)
  // rows of 64 + 16 elements = 160 bytes: by the guide's lane groups the natural ds_read_b128 fragments and both ds_read_b64_tr_b16
  // reads of a transposed fragment are then free of bank conflicts (144-byte rows: 2x the cycles on both; 224-byte rows are free of
  // them too but cost a workgroup per CU).  Measured on one box: dK/dV 311 -> 302 us, forward and dQ unchanged -- the kernels wait on
  // dependencies, not on the LDS array (profiles/r4_ab_attn_lds_row_padding.log).
  static constexpr int PAD = 16;
  using Frag = bf16x8;
  static __device__ __forceinline__ Frag zero() { Frag f; for (int i = 0; i < 8; ++i) f[i] = (bf16)0.f; return f; }
  static __device__ __forceinline__ f32x4 mma(Frag a, Frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct AMma<float> {
  static constexpr int KS = 4;
  static constexpr int PAD = 4;
  using Frag = float;
  static __device__ __forceinline__ Frag zero() { return 0.f; }
  static __device__ __forceinline__ f32x4 mma(Frag a, Frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
};

template <typename T, int HD> struct ACfg {
  static constexpr int KS = AMma<T>::KS;
  static constexpr int HDP = HD > KS ? HD : KS;      // contraction over d padded to one k-step
  static constexpr int LDD = HDP + AMma<T>::PAD;      // [64 tokens][HDP] tiles
  static constexpr int E = 16 / sizeof(T);
  static constexpr int NDS = HDP / KS;                // k-steps of a contraction over d
  static constexpr int TILE = 64 * LDD;               // elements per staged tile
};

// ---- fragments --------------------------------------------------------------------------------------------
// natural-order fragment of a row-major tile: row = row0 + (l&15), k = k0 + [8*(l>>4) .. +7] (bf16) / k0 + (l>>4) (f32)
template <typename T>
__device__ __forceinline__ typename AMma<T>::Frag frag_rows(const T* tile, int ld, int row0, int k0, int l) {
  if constexpr (is_bf16<T>::value) return *(const bf16x8*)(tile + (row0 + (l & 15)) * ld + k0 + 8 * (l >> 4));
  else return tile[(row0 + (l & 15)) * ld + k0 + (l >> 4)];
}
template <typename T>
__device__ __forceinline__ typename AMma<T>::Frag frag_global(const T* rowptr, int k0, int kmax, int l) {
  if constexpr (is_bf16<T>::value) {
    const int k = k0 + 8 * (l >> 4);
    if (k < kmax) return *(const bf16x8*)(rowptr + k);
    return AMma<bf16>::zero();
  } else {
    const int k = k0 + (l >> 4);
    return k < kmax ? rowptr[k] : 0.f;
  }
}
__device__ __forceinline__ float frag_dot(bf16x8 a, bf16x8 b) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += (float)a[i] * (float)b[i];
  return s;
}
__device__ __forceinline__ float frag_dot(float a, float b) { return a * b; }
// bf16: transposed fragment of a row-major [token][d] tile for the contraction over 32 tokens tok0..tok0+31 in the
// ACCUMULATOR slot order (slot j<4 -> token tok0 + 4g + j, j>=4 -> tok0 + 16 + 4g + j-4); MFMA row = d0 + (l&15).
__device__ __forceinline__ bf16x8 frag_tr(const bf16* tile, int ld, int tok0, int d0, int l) {
  const int g = l >> 4, i = l & 15;
  const bf16* a = tile + (tok0 + 4 * g + (i >> 2)) * ld + d0 + 4 * (i & 3);
  bf16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_AS bf16x4*)a);
  bf16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_AS bf16x4*)(a + 16 * ld));
  return __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
}
// The same fragments from an UNPADDED bf16 tile of 64 columns whose 16-byte chunks are XOR-swizzled (chunk c of row r in slot c ^ (r & 7)):
// free of bank conflicts for both kinds of read, and what one LDS-DMA instruction can fill (1 KB = 8 consecutive rows, the swizzle
// applied on the SOURCE side: the lane that fills slot s of row r loads chunk s ^ (r & 7)); the DMA forms of attn_fwd_kernel and
// attn_bwd_q_kernel below.
__device__ __forceinline__ bf16x8 frag_rows_sw(const bf16* tile, int row0, int k0, int l) {
  const int row = row0 + (l & 15), ch = (k0 >> 3) + (l >> 4);
  return *(const bf16x8*)(tile + row * 64 + ((ch ^ (row & 7)) << 3));
}
__device__ __forceinline__ bf16x8 frag_tr_sw(const bf16* tile, int tok0, int d0, int l) {
  const int g = l >> 4, i = l & 15;
  const int row = tok0 + 4 * g + (i >> 2), col = d0 + 4 * (i & 3);
  const bf16* a = tile + row * 64 + (((col >> 3) ^ (row & 7)) << 3) + (col & 4);
  bf16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_AS bf16x4*)a);
  bf16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_AS bf16x4*)(a + 16 * 64));   // (row + 16: the same slot permutation)
  return __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
}
template <typename T, bool SW>
__device__ __forceinline__ typename AMma<T>::Frag frag_rows_x(const T* tile, int ld, int row0, int k0, int l) {
  if constexpr (SW) return frag_rows_sw(tile, row0, k0, l); else return frag_rows<T>(tile, ld, row0, k0, l);
}
template <bool SW>
__device__ __forceinline__ bf16x8 frag_tr_x(const bf16* tile, int ld, int tok0, int d0, int l) {
  if constexpr (SW) return frag_tr_sw(tile, tok0, d0, l); else return frag_tr(tile, ld, tok0, d0, l);
}
__device__ __forceinline__ bf16x8 pack8(f32x4 lo, f32x4 hi) {
  bf16x8 o;
  o[0] = (bf16)lo[0]; o[1] = (bf16)lo[1]; o[2] = (bf16)lo[2]; o[3] = (bf16)lo[3];
  o[4] = (bf16)hi[0]; o[5] = (bf16)hi[1]; o[6] = (bf16)hi[2]; o[7] = (bf16)hi[3];
  return o;
}

// acc[jd] (rows d, col = lane) += X^T[d][tok] * P[tok][lane] for the 64 tokens of a tile, where P[i] are the four
// 16-token accumulator tiles (rows = tokens) and X is the row-major LDS tile [token][d].
template <typename T, int HD>
__device__ __forceinline__ void acc_second_stage(f32x4 (&acc)[HD / 16], const f32x4 (&P)[4], const T* X, int l) {
  using C = ACfg<T, HD>;
  if constexpr (is_bf16<T>::value) {
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      const bf16x8 pf = pack8(P[2 * t2], P[2 * t2 + 1]);
#pragma unroll
      for (int jd = 0; jd < HD / 16; ++jd) acc[jd] = AMma<bf16>::mma(frag_tr(X, C::LDD, 32 * t2, 16 * jd, l), pf, acc[jd]);
    }
  } else {
    const int g = l >> 4, fr = l & 15;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* xr = X + (16 * i + 4 * g + r) * C::LDD + fr;
#pragma unroll
        for (int jd = 0; jd < HD / 16; ++jd) acc[jd] = AMma<float>::mma(xr[16 * jd], P[i][r], acc[jd]);
      }
  }
}

// first stage: S[i] (rows = 16 tokens of tile i, col = lane) = X[tok][:] . f[:]  with f = register fragments of the lane's vector
template <typename T, int HD>
__device__ __forceinline__ void first_stage(f32x4 (&S)[4], const T* X, const typename AMma<T>::Frag (&f)[ACfg<T, HD>::NDS], int l) {
  using C = ACfg<T, HD>;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    S[i] = f32x4{0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < C::NDS; ++s) S[i] = AMma<T>::mma(frag_rows<T>(X, C::LDD, 16 * i, s * C::KS, l), f[s], S[i]);
  }
}

// The same two stages for R query heads that share one kv head (grouped-query attention) and the same 16 tokens per wave: the
// K (V^T, ...) fragment of the staged tile is read from LDS ONCE and feeds R MFMAs.
// (init != nullptr: the chains of block i start from init[i] instead of zero -- the mask as an additive 0 / -1e30, shared by the heads)
template <typename T, int HD, int R, bool SW = false>
__device__ __forceinline__ void first_stage_r(f32x4 (&S)[R][4], const T* X, const typename AMma<T>::Frag (&f)[R][ACfg<T, HD>::NDS], int l,
                                              const f32x4* init = nullptr) {
  using C = ACfg<T, HD>;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int r = 0; r < R; ++r) S[r][i] = init != nullptr ? init[i] : f32x4{0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < C::NDS; ++s) {
      const typename AMma<T>::Frag x = frag_rows_x<T, SW>(X, C::LDD, 16 * i, s * C::KS, l);
#pragma unroll
      for (int r = 0; r < R; ++r) S[r][i] = AMma<T>::mma(x, f[r][s], S[r][i]);
    }
  }
}
template <typename T, int HD, int R, bool SW = false>
__device__ __forceinline__ void acc_second_stage_r(f32x4 (&acc)[R][HD / 16], const f32x4 (&P)[R][4], const T* X, int l) {
  using C = ACfg<T, HD>;
  if constexpr (is_bf16<T>::value) {
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      bf16x8 pf[R];
#pragma unroll
      for (int r = 0; r < R; ++r) pf[r] = pack8(P[r][2 * t2], P[r][2 * t2 + 1]);
#pragma unroll
      for (int jd = 0; jd < HD / 16; ++jd) {
        const bf16x8 x = frag_tr_x<SW>(X, C::LDD, 32 * t2, 16 * jd, l);
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][jd] = AMma<bf16>::mma(x, pf[r], acc[r][jd]);
      }
    }
  } else {
    const int g = l >> 4, fr = l & 15;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const float* xr = X + (16 * i + 4 * g + rr) * C::LDD + fr;
#pragma unroll
        for (int jd = 0; jd < HD / 16; ++jd) {
          const float x = xr[16 * jd];
#pragma unroll
          for (int r = 0; r < R; ++r) acc[r][jd] = AMma<float>::mma(x, P[r][i][rr], acc[r][jd]);
        }
      }
  }
}

// One 16-token block (i) of the first stage / one 32-token half (t2 = blocks 2 t2, 2 t2 + 1) of the second stage: the backward
// kernels need no row maximum (they exponentiate against the stored log-sum-exp), so they run the two stages per half and keep
// only two score blocks per head alive instead of four.
// (S enters with its initial value: zero, or a row / lane constant that the chain then carries -- the dP chains start from -delta, so
// dS = P * (dP - delta) needs no subtraction)
template <typename T, int HD, int R, bool SW = false>
__device__ __forceinline__ void first_stage_block_r(f32x4 (&S)[R], const T* X, const typename AMma<T>::Frag (&f)[R][ACfg<T, HD>::NDS], int i, int l) {
  using C = ACfg<T, HD>;
#pragma unroll
  for (int s = 0; s < C::NDS; ++s) {
    const typename AMma<T>::Frag x = frag_rows_x<T, SW>(X, C::LDD, 16 * i, s * C::KS, l);
#pragma unroll
    for (int r = 0; r < R; ++r) S[r] = AMma<T>::mma(x, f[r][s], S[r]);
  }
}
template <typename T, int HD, int R, bool SW = false>
__device__ __forceinline__ void acc_second_stage_half_r(f32x4 (&acc)[R][HD / 16], const f32x4 (&P)[R][2], const T* X, int t2, int l) {
  using C = ACfg<T, HD>;
  if constexpr (is_bf16<T>::value) {
    bf16x8 pf[R];
#pragma unroll
    for (int r = 0; r < R; ++r) pf[r] = pack8(P[r][0], P[r][1]);
#pragma unroll
    for (int jd = 0; jd < HD / 16; ++jd) {
      const bf16x8 x = frag_tr_x<SW>(X, C::LDD, 32 * t2, 16 * jd, l);
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r][jd] = AMma<bf16>::mma(x, pf[r], acc[r][jd]);
    }
  } else {
    const int g = l >> 4, fr = l & 15;
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const float* xr = X + (16 * (2 * t2 + ii) + 4 * g + rr) * C::LDD + fr;
#pragma unroll
        for (int jd = 0; jd < HD / 16; ++jd) {
          const float x = xr[16 * jd];
#pragma unroll
          for (int r = 0; r < R; ++r) acc[r][jd] = AMma<float>::mma(x, P[r][ii][rr], acc[r][jd]);
        }
      }
  }
}

// ---- staging ----------------------------------------------------------------------------------------------
template <typename T, int HD> struct TileRegs { uint4 v[(64 * HD * sizeof(T) / 16 + 255) / 256]; };

template <typename T, int HD>
__device__ __forceinline__ void tile_store(const TileRegs<T, HD>& r, T* dst, int t) {
  using C = ACfg<T, HD>;
  constexpr int CPR = HD / C::E, N = 64 * CPR;
#pragma unroll
  for (int k = 0; k < (N + 255) / 256; ++k) {
    const int c = t + 256 * k;
    if (c < N) *(uint4*)(dst + (c / CPR) * C::LDD + (c % CPR) * C::E) = r.v[k];
  }
}
// The same tile through a buffer descriptor: the per-thread byte offsets are loop invariant (TileOffs, computed once per kernel), the
// tile's origin is a scalar offset, and rows past the end of the sequence come back as zeros from the descriptor's bounds check --
// no per-load address arithmetic, predicate or zero fill in the staging loops, which are bound by instruction issue
// (profiles/r4_attn_dkv_item_loop_phases.log).
typedef __attribute__((ext_vector_type(4))) int at_i32x4;
extern "C" __device__ at_i32x4 rsys_at_buffer_load_b128(at_i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4i32");
extern "C" __device__ int rsys_at_buffer_load_b32(at_i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.i32");
typedef __attribute__((ext_vector_type(2))) int at_i32x2;
extern "C" __device__ at_i32x2 rsys_at_buffer_load_b64(at_i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v2i32");
// base .. base + bytes is what a load may touch (wave-uniform); bytes < 2^31
__device__ __forceinline__ at_i32x4 at_rsrc(const void* base, long long bytes) {
  const unsigned long long a = (unsigned long long)base;
  at_i32x4 r;
  r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned int)a);
  r[1] = __builtin_amdgcn_readfirstlane((int)(unsigned int)((a >> 32) & 0xFFFFu));   // stride 0
  r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
  r[3] = 0x00020000;                                                               // raw buffer, 32-bit data format
  return r;
}
template <typename T, int HD> struct TileOffs { int v[(64 * HD * sizeof(T) / 16 + 255) / 256]; };
template <typename T, int HD>
__device__ __forceinline__ void tile_offsets(TileOffs<T, HD>& o, long long ld, int t) {
  using C = ACfg<T, HD>;
  constexpr int CPR = HD / C::E, N = 64 * CPR;
#pragma unroll
  for (int k = 0; k < (N + 255) / 256; ++k) {
    const int c = t + 256 * k;
    o.v[k] = c < N ? (int)(((c / CPR) * ld + (c % CPR) * C::E) * (long long)sizeof(T)) : 0x7FFFFFF0;   // (no chunk: out of every range, reads zeros)
  }
}
template <typename T, int HD>
__device__ __forceinline__ void tile_load_buf(TileRegs<T, HD>& r, at_i32x4 rsrc, const TileOffs<T, HD>& o, int soffset) {
  using C = ACfg<T, HD>;
  constexpr int N = 64 * (HD / C::E);
#pragma unroll
  for (int k = 0; k < (N + 255) / 256; ++k) r.v[k] = __builtin_bit_cast(uint4, rsys_at_buffer_load_b128(rsrc, o.v[k], soffset, 0));
}
template <typename T, int HD>
__device__ __forceinline__ void zero_pad_cols(T* dst, int t) {
  using C = ACfg<T, HD>;
  if constexpr (C::HDP > HD) {
    for (int c = t; c < 64 * (C::HDP - HD); c += 256) dst[(c / (C::HDP - HD)) * C::LDD + HD + c % (C::HDP - HD)] = from_f32<T>(0.f);
  }
}
__device__ __forceinline__ int next_bit(unsigned int bits, int from) {  // lowest set bit index >= from, or 32
  const unsigned int m = from >= 32 ? 0u : (bits >> from) << from;
  return m ? __ffs(m) - 1 : 32;
}
__device__ __forceinline__ int next_bit(unsigned long long bits, int from) {  // the same on a wide map word: ... or 64
  const unsigned long long m = from >= 64 ? 0ull : (bits >> from) << from;
  return m ? __ffsll(m) - 1 : 64;
}
// Map words.  A row of up to 32 tiles keeps ONE 32-bit word per map entry (LG = 5: every kernel below is then instruction for instruction
// what it was before rows grew past 2048 tokens); a row of 33 .. 64 tiles keeps one 64-bit word per entry (LG = 6) in the same arrays, which
// are then twice as long (attn_map_words, kernels.hpp).  The launches pick the instantiation from nt alone, so a kernel never meets a map
// of the other width.  LG is also the shift of the dK/dV kernels' item numbers (head of the group << LG | q tile).
template <int LG> struct AMap;
template <> struct AMap<5> { using W = unsigned int; };
template <> struct AMap<6> { using W = unsigned long long; };
template <int LG>
__device__ __forceinline__ typename AMap<LG>::W* map_ptr(unsigned int* m) { return (typename AMap<LG>::W*)m; }
template <int LG>
__device__ __forceinline__ typename AMap<LG>::W map_below(int n) {   // bits 0 .. n - 1
  using W = typename AMap<LG>::W;
  return n >= (1 << LG) ? ~(W)0 : (((W)1 << n) - (W)1);
}
__device__ __forceinline__ unsigned int map_uniform(unsigned int v) { return (unsigned int)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ unsigned long long map_uniform(unsigned long long v) {
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)v), hi = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ int map_popc(unsigned int v) { return __popc(v); }
__device__ __forceinline__ int map_popc(unsigned long long v) { return __popcll(v); }

// ------------------------------------------------------------------------ tile maps
// qmap / qmap_full [b][q tile]: bit j = kv tile j has some / only allowed pairs; kmap* is the transposed relation; the
// *16 maps say the same per group of 16 queries (keys).  One workgroup per (row, q tile); wave w owns the tile's 16
// queries w*16 .. w*16+15 as lane-uniform values (read back from LDS), the lanes sweep the row's keys 64 at a
// time: allowed(q, kv) <=> key[kv] == key[q] or key[kv] == key[q] without its tm bits (token_key below), so a (query,
// 64 keys) step is two compares, an OR and a ballot.  Exact: "some" bits may not miss a pair, "only" bits may not claim one.
__device__ __forceinline__ int token_key(int uid, int tm);
extern "C" __device__ int rsys_at_writelane(int value, int lane, int old) __asm("llvm.amdgcn.writelane.i32");   // v_writelane_b32
template <int LG>
__global__ __launch_bounds__(256) void attn_tilemap_kernel(AttnParams p) {
  using W = typename AMap<LG>::W;
  constexpr int NTM = 1 << LG;   // tiles a map word holds (LG = 6: kcols 32 KB + keys 16 KB of LDS)
  __shared__ W any_bits, any16[4];
  __shared__ unsigned int kany[NTM];            // kany[j]: bit kg = keys 16 kg .. +15 of kv tile j meet a query of this tile
  __shared__ int cnt[NTM];
  __shared__ unsigned short kcols[NTM][64][4];  // [kv tile][key][query group of 16]: the key's bits against this q tile, written out as words
  __shared__ int keys[64 * NTM];                // the row's token keys (one round of loads instead of a dependent load per kv tile)
  __shared__ int qkeys[64];                     // the tile's query keys: read back per query as a lane-uniform VECTOR register (as scalars,
                                                // 16 keys + their tm-less forms + the loop state spilled scalar registers through v_readlane)
  const int qt = blockIdx.x, b = blockIdx.y, t = threadIdx.x, l = t & 63, w = t >> 6;
  const int nt = (p.T + 63) / 64;
  const long long base = (long long)b * p.T;
  if (t == 0) any_bits = 0u;
  if (t < 4) any16[t] = 0u;
  if (t < NTM) { cnt[t] = 0; kany[t] = 0u; }
  for (int i = t; i < nt * 64; i += 256) keys[i] = i < p.T ? token_key(p.uid[base + i], p.tm[base + i]) : KEY_NO_K;
  // lane i < 16 of wave w holds the key of query qt*64 + w*16 + i
  int myq = KEY_NO_Q;
  if (l < 16) { const int q = qt * 64 + w * 16 + l; if (q < p.T) myq = token_key(p.uid[base + q], p.tm[base + q]); }
  if (l < 16) qkeys[w * 16 + l] = myq;
  __syncthreads();
  int aq[16], aq0[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { aq[i] = qkeys[w * 16 + i]; aq0[i] = aq[i] & ~4095; }
  W wany = 0u;
  for (int j = 0; j < nt; ++j) {
    const int ak = keys[j * 64 + l];
    bool mine = false;     // this key meets one of the wave's queries
    int n = 0;             // allowed pairs of this (q group, kv tile), wave-uniform
    unsigned long long qrow = 0ull;   // lane i < 16: the 64 keys of tile j that query w*16 + i may see
    unsigned int kcol = 0u;           // bit i: this lane's key is seen by query w*16 + i
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const bool hit = ak == aq[i] || ak == aq0[i];
      mine |= hit;
      n += __builtin_popcountll(__ballot(hit));
    }
    if (n) {   // (wave-uniform; a (query group, kv tile) pair without an allowed pair keeps zero bits and skips this second pass)
      int qlo = 0, qhi = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const bool hit = ak == aq[i] || ak == aq0[i];
        const unsigned long long hb = __ballot(hit);
        qlo = rsys_at_writelane((int)(unsigned int)hb, i, qlo);            // lane i <- query i's row of key bits
        qhi = rsys_at_writelane((int)(unsigned int)(hb >> 32), i, qhi);
        kcol |= hit ? (1u << i) : 0u;
      }
      qrow = ((unsigned long long)(unsigned int)qhi << 32) | (unsigned int)qlo;
    }
    // the pair bits the attention kernels mask with (AttnParams::qbits / kbits): every (q tile, kv tile), visited or not
    if (l < 16) p.qbits[(((long long)b * nt + qt) * nt + j) * 64 + w * 16 + l] = qrow;
    kcols[j][l][w] = (unsigned short)kcol;
    if (n) {
      wany |= (W)1 << j;
      const unsigned long long km = __ballot(mine);
      unsigned int kg = 0u;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) kg |= ((km >> (16 * g4)) & 0xFFFFull) ? (1u << g4) : 0u;
      if (l == 0) { atomicAdd(&cnt[j], n); atomicOr(&kany[j], kg); }
    }
  }
  if (l == 0) { any16[w] = wany; atomicOr(&any_bits, wany); }
  __syncthreads();
  for (int c = t; c < nt * 64; c += 256)   // kbits[b][kv tile c / 64][qt][key c % 64]: 512-byte runs
    p.kbits[(((long long)b * nt + (c >> 6)) * nt + qt) * 64 + (c & 63)] = *(const unsigned long long*)kcols[c >> 6][c & 63];
  if (t < nt) {
    const bool any = (any_bits >> t) & 1u, full = cnt[t] == 4096;
    if (any) atomicOr(&map_ptr<LG>(p.kmap)[b * nt + t], (W)1 << qt);
    if (full) atomicOr(&map_ptr<LG>(p.kmap_full)[b * nt + t], (W)1 << qt);
    if (full) atomicOr(&map_ptr<LG>(p.qmap_full)[b * nt + qt], (W)1 << t);
    const unsigned int kg = kany[t];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4)
      if ((kg >> g4) & 1u) atomicOr(&map_ptr<LG>(p.kmap16)[(b * nt + t) * 4 + g4], (W)1 << qt);
  }
  if (t == 0) map_ptr<LG>(p.qmap)[b * nt + qt] = any_bits;
  if (t < 4) map_ptr<LG>(p.qmap16)[(b * nt + qt) * 4 + t] = any16[t];
}

// Heaviest-first launch orders (AttnParams::order_q / order_k).  blockIdx.y = 0: the q-side kernels (work of a slot = kv tiles its
// q tile visits; tiles beyond q_active: none), 1: the dK/dV kernel (q tiles its kv tile is visited by).  One workgroup per list of
// attn_work (blockIdx.x = XCD, or the single list of the fallback); rank = slots with more work + equal ones before it (stable, so
// the order is a function of the maps alone).
static int attn_heads_per_wg(const AttnParams& p);
static bool attn_kv_pairs(const AttnParams& p);   // the dK/dV launch of this shape is attn_bwd_kv32_kernel (order_k then lists kv tile PAIRS)
// kv_pairs: the dK/dV side's slots are PAIRS of kv tiles (attn_bwd_kv32_kernel: 128 keys per workgroup), work = q tiles either tile is visited by
// Work keys are 0 .. 2^LG tiles and the padding key 2^LG + 1: rows of OS = 2^LG + 2 counters (34 as before for rows of up to 32 tiles: the same
// stable permutation; 66 for the wide maps, whose chunk cap is halved with it -- attn_order_chunk_cap -- so that the table stays below 64 KB).
static int attn_order_chunk_cap(int lg) { return lg == 5 ? 400 : 200; }
template <int LG>
__global__ __launch_bounds__(256) void attn_order_kernel(AttnParams p, int R, int identity, int kv_pairs) {
  using W = typename AMap<LG>::W;
  constexpr int NTM = 1 << LG, OS = NTM + 2;
  const W *qmap = map_ptr<LG>(p.qmap), *kmap = map_ptr<LG>(p.kmap);
  extern __shared__ int ocnt[];   // [chunks of 64 slots + 1][OS]: slots per (chunk, key), then their exclusive prefixes; last row: totals / bases
  const int side = blockIdx.y, nt = (p.T + 63) / 64, n_groups = p.B * p.KV;
  const int n_inner = side == 0 ? (p.H / p.KV / R) * nt : (kv_pairs ? (nt + 1) / 2 : nt);
  int* out = side == 0 ? p.order_q : p.order_k;
  if (out == nullptr) return;
  const bool lists = (n_groups & 7) == 0;
  const int ns = lists ? (n_groups >> 3) * n_inner : n_groups * n_inner, xcd = blockIdx.x;
  if (!lists && xcd > 0) return;
  out += lists ? xcd * ns : 0;
  if (identity) { for (int sl = threadIdx.x; sl < ns; sl += 256) out[sl] = sl; return; }
  const int nch = (ns + 63) >> 6, l = threadIdx.x & 63, w = threadIdx.x >> 6;
  auto key_of = [&](int sl) -> int {
    if (sl >= ns) return NTM + 1;   // (padding of the last chunk: a key of its own)
    const int group = lists ? (sl / n_inner) * 8 + xcd : sl / n_inner, tile = (sl % n_inner) % nt, b = group / p.KV;
    const int qa = p.q_active != nullptr ? p.q_active[b] : NTM;
    if (side == 0) return tile < qa ? map_popc(qmap[b * nt + tile]) : 0;
    if (kv_pairs) {
      const int t0 = 2 * (sl % n_inner);
      const W u = kmap[b * nt + t0] | (t0 + 1 < nt ? kmap[b * nt + t0 + 1] : (W)0);
      return map_popc(u & map_below<LG>(qa));
    }
    return map_popc(kmap[b * nt + tile] & map_below<LG>(qa));
  };
  auto same_key = [&](int k) -> unsigned long long {   // lanes of this wave that hold the same key
    unsigned long long m = ~0ull;
#pragma unroll
    for (int bit = 0; bit < LG + 1; ++bit) { const unsigned long long bb = __ballot((k >> bit) & 1); m &= ((k >> bit) & 1) ? bb : ~bb; }
    return m;
  };
  for (int i = threadIdx.x; i < (nch + 1) * OS; i += 256) ocnt[i] = 0;
  __syncthreads();
  for (int c = w; c < nch; c += 4) {
    const int k = key_of(c * 64 + l);
    const unsigned long long m = same_key(k);
    if ((m & ((1ull << l) - 1ull)) == 0ull) ocnt[c * OS + k] = __popcll(m);   // (the first lane of each key of the chunk)
  }
  __syncthreads();
  if (threadIdx.x < OS) {
    const int k = threadIdx.x;
    int run = 0;
    for (int c = 0; c < nch; ++c) { const int n = ocnt[c * OS + k]; ocnt[c * OS + k] = run; run += n; }
    ocnt[nch * OS + k] = run;
  }
  __syncthreads();
  if (threadIdx.x == 0) {   // heaviest first: the base of key k = slots with a larger key
    int acc = 0;
    for (int k = NTM; k >= 0; --k) { const int n = ocnt[nch * OS + k]; ocnt[nch * OS + k] = acc; acc += n; }
  }
  __syncthreads();
  for (int c = w; c < nch; c += 4) {
    const int sl = c * 64 + l, k = key_of(sl);
    const unsigned long long m = same_key(k);
    if (sl < ns) out[ocnt[nch * OS + k] + ocnt[c * OS + k] + __popcll(m & ((1ull << l) - 1ull))] = sl;
  }
}

int launch_attn_tilemap(const AttnParams& p, hipStream_t s) {
  ARG_CHECK(p.T % 8 == 0 && (p.T + 63) / 64 <= 64, "attention: T must be a multiple of 8 and <= 4096");
  ARG_CHECK(p.qbits != nullptr && p.kbits != nullptr, "attention: the pair-bit buffers (AttnParams::qbits / kbits) are required");
  const bool wide = (p.T + 63) / 64 > 32;   // 64-bit map words (AMap<6>)
  ARG_CHECK(p.maps_zero_base != nullptr, "attention: the tile maps come from attn_maps_alloc (AttnParams::maps_zero_base)");
  HIP_CHECK(hipMemsetAsync(p.maps_zero_base, 0, p.maps_zero_bytes, s));
  if (wide) hipLaunchKernelGGL(attn_tilemap_kernel<6>, dim3((p.T + 63) / 64, p.B), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(attn_tilemap_kernel<5>, dim3((p.T + 63) / 64, p.B), dim3(256), 0, s, p);
  if (p.order_q != nullptr || p.order_k != nullptr) {
    const int R = attn_heads_per_wg(p), nt = (p.T + 63) / 64, n_groups = p.B * p.KV;
    const int ns_max = ((n_groups & 7) == 0 ? (n_groups >> 3) : n_groups) * (p.H / p.KV) * nt;
    // (a list beyond one workgroup's LDS: keep the plain order -- the kernels read an identity permutation)
    const int cap = attn_order_chunk_cap(wide ? 6 : 5), nch = (ns_max + 63) / 64;
    const dim3 og((n_groups & 7) == 0 ? 8 : 1, 2);
    if (wide) hipLaunchKernelGGL(attn_order_kernel<6>, og, dim3(256), (size_t)(std::min(nch, cap) + 1) * 66 * 4, s, p, R, nch > cap ? 1 : 0, attn_kv_pairs(p) ? 1 : 0);
    else hipLaunchKernelGGL(attn_order_kernel<5>, og, dim3(256), (size_t)(std::min(nch, cap) + 1) * 34 * 4, s, p, R, nch > cap ? 1 : 0, attn_kv_pairs(p) ? 1 : 0);
  }
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}

// allowed(q, kv) = uid equal AND (tm[kv] == 0 OR tm equal).  With the token key a = uid << 12 | tm (host-checked:
// 0 <= uid < 2^19, 0 <= tm < 4096) this is  a[kv] == (a[q] & ~4095)  OR  a[kv] == a[q].  The compares run ONCE per step and map set, in
// attn_tilemap_kernel, which keeps their outcome as pair bits (AttnParams::qbits / kbits); the attention kernels mask from those.
__device__ __forceinline__ int token_key(int uid, int tm) { return (int)(((unsigned int)uid << 12) | (unsigned int)tm); }
// Masks from the precomputed pair bits: `word` = the lane's 64-bit row of the (q tile, kv tile) bit matrix, already shifted right by
// 4 g, so that the partner of the lane's score (block i, register rr) is bit 16 i + rr: a signed one-bit extract gives 0 / -1 and a
// bit-field insert picks the score or the fill -- two VALU instructions per score, the extract shared by the R heads, no key reads.
template <int R>
__device__ __forceinline__ void mask_bits_block(f32x4 (&S)[R], unsigned long long word, int i, float fill) {
  const int src = (int)(i < 2 ? (unsigned int)word : (unsigned int)(word >> 32));
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int m = __builtin_amdgcn_sbfe(src, 16 * (i & 1) + rr, 1);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float sv = S[r][rr];   // (a copy: __builtin_bit_cast of a vector ELEMENT reads element 0 with this compiler)
      S[r][rr] = __builtin_bit_cast(float, (__builtin_bit_cast(int, sv) & m) | (__builtin_bit_cast(int, fill) & ~m));
    }
  }
}
// The same mask as an ADDEND: 0 where the pair is allowed, -1e30 where not.  A score chain that starts from it ends at exactly the value
// mask_bits_block would have put there (-1e30 + q.k = -1e30 in fp32), costs no instruction per head, and the addend is the same for every
// head of the workgroup: extract + insert once per score position instead of extract + one insert per head.
__device__ __forceinline__ f32x4 mask_bias_block(unsigned long long word, int i) {
  const int src = (int)(i < 2 ? (unsigned int)word : (unsigned int)(word >> 32));
  f32x4 b;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int m = __builtin_amdgcn_sbfe(src, 16 * (i & 1) + rr, 1);
    b[rr] = __builtin_bit_cast(float, __builtin_bit_cast(int, -1e30f) & ~m);
  }
  return b;
}
// XCD-aware work mapping.  Workgroups are dealt round-robin over the 8 XCDs (private L2 each); all workgroups of one
// (row, kv head) group read the same K/V (forward, dQ) or Q/dO (dK/dV) tiles, so a group is kept on ONE XCD: its tiles
// are fetched from HBM once instead of once per XCD (rocprofv3 FETCH_SIZE: 2.9x the algorithmic bytes before).
// 1-D grid of n_groups * n_inner workgroups; falls back to the plain order when n_groups is not a multiple of 8.
// order (optional): per XCD list (or one list in the fallback) the slots sorted heaviest first (attn_order_kernel): workgroups are
// dispatched in blockIdx order, so the long ones start first and the short ones fill the tail of the launch.
__device__ __forceinline__ void attn_work(int n_groups, int n_inner, const int* __restrict__ order, int& group, int& inner) {
  const int bid = blockIdx.x;
  if ((n_groups & 7) == 0) {
    const int xcd = bid & 7;
    int slot = bid >> 3;
    if (order != nullptr) slot = order[xcd * ((n_groups >> 3) * n_inner) + slot];
    group = (slot / n_inner) * 8 + xcd;
    inner = slot % n_inner;
  } else {
    const int slot = order != nullptr ? order[bid] : bid;
    group = slot / n_inner;
    inner = slot % n_inner;
  }
}

// largest magnitude among the elements of one 16-byte chunk of a T tile (fp8 trunk: amax of a tensor while it is written)
template <typename T>
__device__ __forceinline__ float chunk_amax(const uint4& v) {
  if constexpr (is_bf16<T>::value) {
    const bf16x8 h = __builtin_bit_cast(bf16x8, v);
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) m = fmaxf(m, fabsf((float)h[k]));
    return m;
  } else {
    const float4 f = __builtin_bit_cast(float4, v);
    return fmaxf(fmaxf(fabsf(f.x), fabsf(f.y)), fmaxf(fabsf(f.z), fabsf(f.w)));
  }
}
template <typename T, int HD>
__device__ __forceinline__ void copy_out_tile(const T* Os, T* dst, long long ld, int tile_tok0, int T_len, int t, float* amax = nullptr) {
  using C = ACfg<T, HD>;
  constexpr int CPR = HD / C::E;
  float am = 0.f;
  for (int c = t; c < 64 * CPR; c += 256) {
    const int row = c / CPR, ch = c % CPR;
    if (tile_tok0 + row < T_len) {
      const uint4 v = *(const uint4*)(Os + row * C::LDD + ch * C::E);
      *(uint4*)(dst + (long long)row * ld + ch * C::E) = v;
      if (amax != nullptr) am = fmaxf(am, chunk_amax<T>(v));
    }
  }
  if (amax != nullptr) {
    am = wave_max(am);
    if ((t & 63) == 0) f8_amax_add(amax, am);
  }
}

extern "C" __device__ void rsys_at_buffer_load_lds(at_i32x4 rsrc, LDS_AS unsigned int* lds, int size, int voffset, int soffset, int offset,
                                                   int aux) __asm("llvm.amdgcn.raw.buffer.load.lds");
// The same instruction behind an asm statement (ATTN_DMA_ASM): the compiler's wait-count pass orders every LDS read that it cannot tell
// apart from a pending LDS-DMA behind that DMA, i.e. it would make an item wait for the NEXT item's tiles as soon as it reads LDS.  Here
// it does not see the DMA; vector memory returns in issue order, so its own counted waits for later loads still cover what they must, and
// the wave's explicit s_waitcnt vmcnt(0) before the publishing barrier covers the DMA.  lds: wave-uniform LDS byte address.
// (M0 is written here and listed as clobbered, so that the compiler never takes an M0 value of its own for still valid behind the statement;
// clang's warning about a reserved register on the clobber list is silenced for this one statement: the clobber is the intent.)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void dma16_asm(at_i32x4 rsrc, unsigned int lds, int voffset, int soffset) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lds), "v"(voffset), "s"(rsrc), "s"(soffset) : "memory", "m0");
}
#pragma clang diagnostic pop
// (Measured per kernel on one box in round 4, intrinsic -> asm: dK/dV 193 -> 183 us, dQ 171 -> 177, forward 123 -> 127.  Round 5 found why the
// query-side kernels lost: their Q / dO fragment loads were still PENDING in the compiler's bookkeeping when the item loop began, so its
// wait-count pass kept counted vmcnt waits for them inside the loop -- counts that do not include the asm DMA, so each drained the
// next item's tiles; with those loads retired in front of the loop (an empty asm that names the registers) the asm form has no vector-memory
// wait between an item's first MFMA and its publishing wait, where the intrinsic form has a vmcnt(0) after the first third of the item.)
#ifndef ATTN_QSIDE_DMA_ASM
#define ATTN_QSIDE_DMA_ASM true
#endif
template <bool ASM>
__device__ __forceinline__ void dma16(at_i32x4 rsrc, unsigned char* lds, int voffset, int soffset) {
  if constexpr (ASM) dma16_asm(rsrc, (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(unsigned long long)(LDS_AS unsigned char*)lds), voffset, soffset);
  else rsys_at_buffer_load_lds(rsrc, (LDS_AS unsigned int*)lds, 16, voffset, soffset, 0, 0);
}
// 32 x 32 x 16 products (the 32-token-per-wave kernel attn_bwd_kv32_kernel; LDS image and fragment maps: see there)
typedef __attribute__((ext_vector_type(16))) float f32x16;
__device__ __forceinline__ int sw32(int r) { return (((r >> 1) & 1) << 2) | (((r >> 2) & 1) << 1) | ((r >> 3) & 1); }
__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ bf16x8 pack8f(const f32x16& v, int o) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (bf16)v[o + j];
  return r;
}
// ------------------------------------------------------------------------ forward
// R = query heads per workgroup: the R heads of one kv head's group at the SAME 64 tokens (R = 1: one head).  They share the
// staged K / V tile, every K and V^T fragment read, the tile maps and -- the mask depends on the tokens only -- the mask
// predicates; soft-max statistics and the output accumulators are per head.
// DMA (bf16, head_dim 64): the K / V tiles arrive by LDS-DMA in unpadded XOR-swizzled tiles (frag_rows_sw).
template <typename T, int HD, int R, bool DMA = false, int LG = 5>
__global__ __launch_bounds__(256, (is_bf16<T>::value && HD <= 64) ? (R == 1 ? 3 : (DMA ? 3 : 2)) : 1) void attn_fwd_kernel(AttnParams p) {
  using C = ACfg<T, HD>;
  using W = typename AMap<LG>::W;
  using M = AMma<T>;
  static_assert(!DMA || (is_bf16<T>::value && HD == 64), "LDS-DMA staging: bf16, head_dim 64");
  constexpr int TILE = DMA ? 64 * 64 : C::TILE;   // elements of a staged tile
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* Ks = (T*)smem_raw;                       // [2][64][LDD]   (DMA: [2][64][64] swizzled)
  T* Vs = Ks + 2 * TILE;                      // [2][64][LDD]
  unsigned long long* ab = (unsigned long long*)(Vs + 2 * TILE);   // [2][64] pair bits of the 64 queries against the staged tile's keys
  const int nt = (p.T + 63) / 64;
  int grp, inner;
  attn_work(p.B * p.KV, (p.H / p.KV / R) * nt, p.order_q, grp, inner);
  const int b = grp / p.KV, kvh = grp % p.KV, h0 = kvh * (p.H / p.KV) + (inner / nt) * R, qt = inner % nt;
  if (p.q_active != nullptr && qt >= p.q_active[b]) return;   // nobody reads this query tile's output (uniform: whole workgroup)
  const int t = threadIdx.x, l = t & 63, w = t >> 6, g = l >> 4, fr = l & 15;
  const long long tok0 = (long long)b * p.T;
  const float c2 = rsqrtf((float)HD) * LOG2E;        // scores are handled in log2 units
  const int q = qt * 64 + w * 16 + fr;               // this lane's query
  const bool qv = q < p.T;
  typename M::Frag qf[R][C::NDS];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const T* qrow = (const T*)p.q + (tok0 + min(q, p.T - 1)) * p.ld + (h0 + r) * HD;
#pragma unroll
    for (int s = 0; s < C::NDS; ++s) qf[r][s] = frag_global<T>(qrow, s * C::KS, HD, l);
  }
  float m_run[R], l_run[R];
  f32x4 oacc[R][HD / 16];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    m_run[r] = -1e30f; l_run[r] = 0.f;
#pragma unroll
    for (int j = 0; j < HD / 16; ++j) oacc[r][j] = f32x4{0, 0, 0, 0};
  }
  if constexpr (!DMA) { zero_pad_cols<T, HD>(Ks, t); zero_pad_cols<T, HD>(Ks + C::TILE, t); }
  // (scalars through readfirstlane: loaded by vector memory -- the maps are not const -- and otherwise still pending when the item loop begins)
  const W bits = map_uniform(map_ptr<LG>(p.qmap)[b * nt + qt]), fullbits = map_uniform(map_ptr<LG>(p.qmap_full)[b * nt + qt]);
  const W wbits = map_uniform(map_ptr<LG>(p.qmap16)[(b * nt + qt) * 4 + w]);   // kv tiles this wave's 16 queries take part in
  // K / V of this kv head, rows of this sequence ([T][HD] windows of the row-major qkv), and the rows' uid / tm (tile_load_buf)
  const at_i32x4 k_rs = at_rsrc((const T*)p.k + tok0 * p.ld + kvh * HD, ((long long)(p.T - 1) * p.ld + HD) * sizeof(T));
  const at_i32x4 v_rs = at_rsrc((const T*)p.v + tok0 * p.ld + kvh * HD, ((long long)(p.T - 1) * p.ld + HD) * sizeof(T));
  // the pair bits of this q tile against every kv tile: [nt][64 queries] words (AttnParams::qbits)
  const at_i32x4 qb_rs = at_rsrc(p.qbits + ((long long)b * nt + qt) * nt * 64, (long long)nt * 64 * 8);
  TileOffs<T, HD> kv_of;
  tile_offsets<T, HD>(kv_of, p.ld, t);
  const bool w0 = __builtin_amdgcn_readfirstlane(w) == 0;

  TileRegs<T, HD> rk, rv;
  unsigned long long rb = 0ull;
  int dv_[2] = {0, 0};   // DMA: wave w fills rows 16 w .. + 15 of a tile with two instructions (8 rows each); per-lane source offsets
  if constexpr (DMA) {
#pragma unroll
    for (int k = 0; k < 2; ++k) { const int row = 16 * w + 8 * k + (l >> 3); dv_[k] = (int)((row * p.ld + ((l & 7) ^ (row & 7)) * 8) * sizeof(T)); }
  }
  auto gload = [&](int kt, int buf) {   // (DMA: straight into buffer buf; else into registers, lstore(buf) follows after the arithmetic)
    const int so = (int)(kt * 64 * p.ld * sizeof(T));
    if constexpr (DMA) {
      unsigned char* kd = (unsigned char*)(Ks + buf * TILE) + (16 * w) * 128;
      unsigned char* vd = (unsigned char*)(Vs + buf * TILE) + (16 * w) * 128;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        dma16<ATTN_QSIDE_DMA_ASM>(k_rs, kd + k * 1024, dv_[k], so);
        dma16<ATTN_QSIDE_DMA_ASM>(v_rs, vd + k * 1024, dv_[k], so);
      }
    } else {
      tile_load_buf<T, HD>(rk, k_rs, kv_of, so);
      tile_load_buf<T, HD>(rv, v_rs, kv_of, so);
    }
    if (w0) rb = __builtin_bit_cast(unsigned long long, rsys_at_buffer_load_b64(qb_rs, 8 * l, kt * 512, 0));   // query l's keys of tile kt
  };
  auto lstore = [&](int buf) {
    if constexpr (!DMA) {
      tile_store<T, HD>(rk, Ks + buf * TILE, t);
      tile_store<T, HD>(rv, Vs + buf * TILE, t);
    }
    if (w0) ab[buf * 64 + l] = rb;
    if constexpr (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA landed (the barrier follows)
  };

  int kt = next_bit(bits, 0);
  int cur = 0;
  if (kt < nt) { gload(kt, 0); lstore(0); }
  if constexpr (DMA && ATTN_QSIDE_DMA_ASM) {   // retire the Q fragments' loads in the compiler's bookkeeping before the loop (see dma16)
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int s = 0; s < C::NDS; ++s) asm volatile("" : "+v"(qf[r][s]));
  }
  __syncthreads();
  while (kt < nt) {
    const int nxt = next_bit(bits, kt + 1);
    if (nxt < nt) gload(nxt, cur ^ 1);
    const T* Kc = Ks + cur * TILE;
    const T* Vc = Vs + cur * TILE;
    if ((wbits >> kt) & 1u) {   // (a wave whose 16 queries have no allowed key in this tile leaves its state untouched)
    f32x4 S[R][4];
    if (!((fullbits >> kt) & 1u)) {
      // the lane's query against the tile's 64 keys (pair bits): the mask enters the score chains as their starting value
      const unsigned long long wq = ab[cur * 64 + w * 16 + fr] >> (4 * g);
      f32x4 bias[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) bias[i] = mask_bias_block(wq, i);
      first_stage_r<T, HD, R, DMA>(S, Kc, qf, l, bias);
    } else {
      first_stage_r<T, HD, R, DMA>(S, Kc, qf, l);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float tmax = -1e30f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) tmax = fmaxf(tmax, S[r][i][rr]);
      tmax = quad_rows_max(tmax);
      const float m_new = fmaxf(m_run[r], tmax * c2);
      const float mu_old = fmaxf(m_run[r], -1e20f), mu_new = fmaxf(m_new, -1e20f);
      const float alpha = fexp2(mu_old - mu_new);
      float psum = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const float pv = fexp2(fmaf(S[r][i][rr], c2, -mu_new));   // masked entries: exp2(-1.8e29) = 0
          S[r][i][rr] = pv;
          psum += pv;
        }
      psum = quad_rows_sum(psum);
      l_run[r] = l_run[r] * alpha + psum;
      m_run[r] = m_new;
#pragma unroll
      for (int j = 0; j < HD / 16; ++j) oacc[r][j] *= alpha;
    }
    acc_second_stage_r<T, HD, R, DMA>(oacc, S, Vc, l);
    }
    if (nxt < nt) lstore(cur ^ 1);
    __syncthreads();
    cur ^= 1;
    kt = nxt;
  }
  // O^T (rows d, col q) -> row-major through LDS (head r in the r-th staged-tile slot), then 16-byte row stores
#pragma unroll
  for (int r = 0; r < R; ++r) {
    T* Os = Ks + r * C::TILE;   // [64][LDD]   (R <= 4: the four staged-tile slots)
    const float inv = l_run[r] > 0.f ? 1.f / l_run[r] : 0.f;
#pragma unroll
    for (int j = 0; j < HD / 16; ++j) {
      T* dst = Os + (w * 16 + fr) * C::LDD + 16 * j + 4 * g;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) dst[rr] = from_f32<T>(oacc[r][j][rr] * inv);
    }
    if (g == 0 && qv) p.lse[((long long)b * p.H + h0 + r) * p.T + q] = (m_run[r] + log2f(l_run[r])) * (1.f / LOG2E);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < R; ++r)
    copy_out_tile<T, HD>(Ks + r * C::TILE, (T*)p.o + (tok0 + qt * 64) * p.ldo + (h0 + r) * HD, p.ldo, qt * 64, p.T, t, p.f8_amax);
}


// query heads per workgroup of the forward / dQ kernels: the whole group of a kv head when that is 2 (every configuration of
// H / KV = 2), else 1.
static bool attn_dma_on() { return sw().attn_dma != 0; }
static int attn_heads_per_wg(const AttnParams& p) {
  return (p.H / p.KV == 2 && p.hd <= 64) ? 2 : 1;   // (head_dim 128: two heads' accumulators cost a wave per SIMD)
}

template <typename T, int HD, int LG>
static int attn_fwd_hd(const AttnParams& p, hipStream_t s) {
  using C = ACfg<T, HD>;
  const size_t sm = sizeof(T) * 4 * C::TILE + 384 * sizeof(int);
  static bool set = false;
  if (!set) {
    HIP_CHECK(hipFuncSetAttribute((const void*)attn_fwd_kernel<T, HD, 1, false, LG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    HIP_CHECK(hipFuncSetAttribute((const void*)attn_fwd_kernel<T, HD, 2, false, LG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    set = true;
  }
  if constexpr (is_bf16<T>::value && HD == 64) {
    if (attn_dma_on()) {   // LDS-DMA staging (RSYS_ATTN_DMA=0: the register-staged kernels)
      const size_t sm_dma = 4 * 64 * 64 * 2 + 384 * 4;
      if (attn_heads_per_wg(p) == 2) hipLaunchKernelGGL((attn_fwd_kernel<T, HD, 2, true, LG>), dim3(((p.T + 63) / 64) * (p.H / 2) * p.B), dim3(256), sm_dma, s, p);
      else hipLaunchKernelGGL((attn_fwd_kernel<T, HD, 1, true, LG>), dim3(((p.T + 63) / 64) * p.H * p.B), dim3(256), sm_dma, s, p);
      HIP_CHECK(hipGetLastError());
      return RSYS_OK;
    }
  }
  if (attn_heads_per_wg(p) == 2) hipLaunchKernelGGL((attn_fwd_kernel<T, HD, 2, false, LG>), dim3(((p.T + 63) / 64) * (p.H / 2) * p.B), dim3(256), sm, s, p);
  else hipLaunchKernelGGL((attn_fwd_kernel<T, HD, 1, false, LG>), dim3(((p.T + 63) / 64) * p.H * p.B), dim3(256), sm, s, p);
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}

static int check_attn(const AttnParams& p, size_t esz) {
  ARG_CHECK(p.T % 8 == 0 && (p.T + 63) / 64 <= 64, "attention: T must be a multiple of 8 and <= 4096");
  ARG_CHECK(p.qbits != nullptr && p.kbits != nullptr, "attention: the pair-bit buffers (AttnParams::qbits / kbits) are required");
  ARG_CHECK(p.H % p.KV == 0, "attention: H % KV");
  ARG_CHECK((p.ld * esz) % 16 == 0 && (p.hd * esz) % 16 == 0, "attention: 16-byte row alignment");
  // (the kernels address a row's tiles through 32-bit buffer offsets: at T = 4096, ld = 4096 in bf16 a row is 32 MiB)
  ARG_CHECK((long long)p.T * std::max(p.ld, p.ldo) * (long long)esz < (1ll << 31), "attention: a row of qkv must stay below 2 GiB");
  return RSYS_OK;
}

template <typename T>
int launch_attn_fwd(const AttnParams& p, hipStream_t s) {
  int rc = check_attn(p, sizeof(T));
  if (rc) return rc;
  const bool wide = (p.T + 63) / 64 > 32;   // 64-bit map words: the AMap<6> instantiations (rows of up to 32 tiles keep the 32-bit ones)
  switch (p.hd) {
    case 16: return wide ? attn_fwd_hd<T, 16, 6>(p, s) : attn_fwd_hd<T, 16, 5>(p, s);
    case 32: return wide ? attn_fwd_hd<T, 32, 6>(p, s) : attn_fwd_hd<T, 32, 5>(p, s);
    case 64: return wide ? attn_fwd_hd<T, 64, 6>(p, s) : attn_fwd_hd<T, 64, 5>(p, s);
    case 128: return wide ? attn_fwd_hd<T, 128, 6>(p, s) : attn_fwd_hd<T, 128, 5>(p, s);
  }
  set_error("attention: head_dim must be 16, 32, 64 or 128");
  return RSYS_ERR_ARG;
}
template int launch_attn_fwd<bf16>(const AttnParams&, hipStream_t);
template int launch_attn_fwd<float>(const AttnParams&, hipStream_t);


// gradient tile (rows d = 16j+4g+r, col = token on the lane) -> un-rotate (inverse of transformer.model.py:182-190; the
// pair (d, d+1) is two consecutive registers of the lane), transpose through LDS, store rows with 16-byte accesses
template <typename T, int HD>
__device__ __forceinline__ void store_grad_tile(f32x4 (&acc)[HD / 16], bool rotate, const float* rope_cos, const float* rope_sin,
                                                int pos, T* Os, int w, int l) {
  using C = ACfg<T, HD>;
  const int g = l >> 4, fr = l & 15;
#pragma unroll
  for (int j = 0; j < HD / 16; ++j) {
    float o[4] = {acc[j][0], acc[j][1], acc[j][2], acc[j][3]};
    if (rotate) {
      const int d2 = (16 * j + 4 * g) >> 1;
      const float2 cc = *(const float2*)(rope_cos + pos * (HD / 2) + d2);
      const float2 ss = *(const float2*)(rope_sin + pos * (HD / 2) + d2);
      const float a0 = o[0] * cc.x + o[1] * ss.x, a1 = -o[0] * ss.x + o[1] * cc.x;
      const float b0 = o[2] * cc.y + o[3] * ss.y, b1 = -o[2] * ss.y + o[3] * cc.y;
      o[0] = a0; o[1] = a1; o[2] = b0; o[3] = b1;
    }
    T* dst = Os + (w * 16 + fr) * C::LDD + 16 * j + 4 * g;
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[r] = from_f32<T>(o[r]);
  }
}
// ------------------------------------------------------------------------ backward: dK, dV (one workgroup per kv tile and kv head)
template <typename T, int HD, int LG = 5>
__global__ __launch_bounds__(256, (is_bf16<T>::value && HD <= 64) ? 3 : 1) void attn_bwd_kv_kernel(AttnParams p) {
  using C = ACfg<T, HD>;
  using M = AMma<T>;
  using W = typename AMap<LG>::W;
  constexpr int NTM = 1 << LG;   // item = head of the group * NTM + q tile
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* Qs = (T*)smem_raw;                  // [2][64 q][LDD]
  T* dOs = Qs + 2 * C::TILE;             // [2][64 q][LDD]
  float* lse2 = (float*)(dOs + 2 * C::TILE);   // [2][64]
  float* dls = lse2 + 128;                      // [2][64]
  unsigned long long* kbs = (unsigned long long*)(dls + 128);   // [2][64] pair bits of the 64 keys against the staged item's queries
  const int rep = p.H / p.KV, nt = (p.T + 63) / 64;
  int grp, kvt;
  attn_work(p.B * p.KV, nt, p.order_k, grp, kvt);
  const int b = grp / p.KV, kvh = grp % p.KV;
  const int t = threadIdx.x, l = t & 63, w = t >> 6, g = l >> 4, fr = l & 15;
  const long long tok0 = (long long)b * p.T;
  const float scale = rsqrtf((float)HD), c2 = scale * LOG2E;
  const int kv = kvt * 64 + w * 16 + fr;       // this lane's key/value token
  const bool kvv = kv < p.T;
  typename M::Frag kf[1][C::NDS], vf[1][C::NDS];
  {
    const T* krow = (const T*)p.k + (tok0 + min(kv, p.T - 1)) * p.ld + kvh * HD;
    const T* vrow = (const T*)p.v + (tok0 + min(kv, p.T - 1)) * p.ld + kvh * HD;
#pragma unroll
    for (int s = 0; s < C::NDS; ++s) { kf[0][s] = frag_global<T>(krow, s * C::KS, HD, l); vf[0][s] = frag_global<T>(vrow, s * C::KS, HD, l); }
  }
  f32x4 dK[1][HD / 16], dV[1][HD / 16];
#pragma unroll
  for (int j = 0; j < HD / 16; ++j) { dK[0][j] = f32x4{0, 0, 0, 0}; dV[0][j] = f32x4{0, 0, 0, 0}; }
  for (int i = 0; i < 2; ++i) { zero_pad_cols<T, HD>(Qs + i * C::TILE, t); zero_pad_cols<T, HD>(dOs + i * C::TILE, t); }
  const int qa = p.q_active != nullptr ? p.q_active[b] : NTM;
  const W act = map_below<LG>(qa);   // query tiles whose dO can be non-zero
  const W bits = map_ptr<LG>(p.kmap)[b * nt + kvt] & act, fullbits = map_ptr<LG>(p.kmap_full)[b * nt + kvt];
  const W wbits = map_uniform(map_ptr<LG>(p.kmap16)[(b * nt + kvt) * 4 + w]);   // q tiles that may see this wave's 16 keys

  // Staging runs TWO items ahead of the arithmetic: an item's global loads have a whole iteration (one item of another workgroup's
  // arithmetic would not cover their latency) before they are stored to LDS, and that store is in LDS one barrier before its use.
  // Two register sets, used alternately (the loop below is unrolled by two so that each stays in fixed registers).
  struct ItemRegs { TileRegs<T, HD> rq, rdo; int x, y; unsigned long long kb; };   // (wave 0) x, y: log-sum-exp and -delta of query l; kb: pair bits of key l
  ItemRegs R0, R1;
  R0.x = R1.x = R0.y = R1.y = 0; R0.kb = R1.kb = 0ull;
  // Q / dO of the kv head's query heads, rows of this sequence: [T][rep * HD] windows of the row-major tensors
  const at_i32x4 q_rs = at_rsrc((const T*)p.q + tok0 * p.ld + kvh * rep * HD, ((long long)(p.T - 1) * p.ld + rep * HD) * sizeof(T));
  const at_i32x4 do_rs = at_rsrc((const T*)p.dO + tok0 * p.ldo + kvh * rep * HD, ((long long)(p.T - 1) * p.ldo + rep * HD) * sizeof(T));
  TileOffs<T, HD> q_of, do_of;
  tile_offsets<T, HD>(q_of, p.ld, t);
  tile_offsets<T, HD>(do_of, p.ldo, t);
  // [rep][T] windows of lse / delta (a row past T of a head reads the next head's, finite and masked; of the last head: zero), [T] of uid / tm
  const at_i32x4 lse_rs = at_rsrc(p.lse + ((long long)b * p.H + kvh * rep) * p.T, (long long)rep * p.T * 4);
  const at_i32x4 dl_rs = at_rsrc(p.delta + ((long long)b * p.H + kvh * rep) * p.T, (long long)rep * p.T * 4);
  // the pair bits of this kv tile against every q tile: [nt][64 keys] words (AttnParams::kbits)
  const at_i32x4 kb_rs = at_rsrc(p.kbits + ((long long)b * nt + kvt) * nt * 64, (long long)nt * 64 * 8);
  // wave 0 (a wave-uniform branch) stages the 64 rows' scalars.  (One array per wave instead -- log-sum-exp, -delta, keys on waves 0, 1, 2 --
  // was measured 7 % SLOWER: three more uniform branches per item in every wave; profiles/r4_ab_attn_staging.log)
  const bool w0 = __builtin_amdgcn_readfirstlane(w) == 0;
  auto gload = [&](ItemRegs& r, int it) {   // it = head-in-group * NTM + q tile
    const int hh = it >> LG, qt = it & (NTM - 1);
    tile_load_buf<T, HD>(r.rq, q_rs, q_of, (int)((qt * 64 * p.ld + hh * HD) * sizeof(T)));
    tile_load_buf<T, HD>(r.rdo, do_rs, do_of, (int)((qt * 64 * p.ldo + hh * HD) * sizeof(T)));
    if (w0) {   // (rows past the sequence: the next head's finite values or zero, all masked, and the key of no query)
      const int so = (hh * p.T + qt * 64) * 4;
      r.x = __builtin_bit_cast(int, __builtin_bit_cast(float, rsys_at_buffer_load_b32(lse_rs, 4 * l, so, 0)) * LOG2E);
      r.y = rsys_at_buffer_load_b32(dl_rs, 4 * l, so, 0) ^ 0x80000000;   // -delta: what the dP chains start from
      r.kb = __builtin_bit_cast(unsigned long long, rsys_at_buffer_load_b64(kb_rs, 8 * l, qt * 512, 0));   // key l against the 64 queries
    }
  };
  auto lstore = [&](const ItemRegs& r, int buf) {
    tile_store<T, HD>(r.rq, Qs + buf * C::TILE, t);
    tile_store<T, HD>(r.rdo, dOs + buf * C::TILE, t);
    if (w0) { ((int*)lse2)[buf * 64 + l] = r.x; ((int*)dls)[buf * 64 + l] = r.y; kbs[buf * 64 + l] = r.kb; }
  };
  auto next_item = [&](int from) {   // items are (head, q tile) pairs in order; returns rep * NTM when exhausted
    int hh = from >> LG, qt = from & (NTM - 1);
    while (hh < rep) {
      const int n = next_bit(bits, qt);
      if (n < nt) return hh * NTM + n;
      ++hh; qt = 0;
    }
    return rep * NTM;
  };
  const int end = rep * NTM;
  int it = next_item(0), cur = 0;
  int nxt = it < end ? next_item(it + 1) : end, nxt2 = nxt < end ? next_item(nxt + 1) : end;   // the items staged one and two ahead
  if (it < end) { gload(R0, it); lstore(R0, 0); }
  if (nxt < end) gload(R1, nxt);
  __syncthreads();
  auto step = [&](ItemRegs& rload, const ItemRegs& rstore) {   // rstore holds item nxt; item nxt2 is loaded into rload
    if (nxt2 < end) gload(rload, nxt2);
    const T* Qc = Qs + cur * C::TILE;
    const T* dOc = dOs + cur * C::TILE;
    if ((wbits >> (it & (NTM - 1))) & 1u) {   // (nothing to add for a wave whose 16 keys no query of this tile may see)
    const bool fullt = (fullbits >> (it & (NTM - 1))) & 1u;
    const unsigned long long wk = kbs[cur * 64 + w * 16 + fr] >> (4 * g);   // the lane's key against the item's 64 queries (mask_bits_block)
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {   // 32 queries at a time: both stages, two score blocks alive (no row maximum is needed here)
      f32x4 P2[1][2], dS2[1][2];
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
        const int i = 2 * t2 + ii;
        const float4 l4 = *(const float4*)(lse2 + cur * 64 + 16 * i + 4 * g);
        const float4 d4 = *(const float4*)(dls + cur * 64 + 16 * i + 4 * g);
        const float ll[4] = {l4.x, l4.y, l4.z, l4.w};
        f32x4 S[1] = {f32x4{0, 0, 0, 0}}, dP[1] = {f32x4{d4.x, d4.y, d4.z, d4.w}};   // (rows = queries: the chain starts from -delta[q])
        first_stage_block_r<T, HD, 1>(S, Qc, kf, i, l);      // S[q][kv]: rows q (registers), col kv (lane)
        first_stage_block_r<T, HD, 1>(dP, dOc, vf, i, l);    // dP[q][kv] - delta[q]
        if (!fullt) mask_bits_block<1>(S, wk, i, -1e30f);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pv = fexp2(fmaf(S[0][r], c2, -ll[r]));   // masked: exp2(-1.8e29 - lse) = 0
          P2[0][ii][r] = pv;
          dS2[0][ii][r] = pv * dP[0][r];   // (the 1/sqrt(hd) factor of dS is applied once to dK at the end)
        }
      }
      acc_second_stage_half_r<T, HD, 1>(dV, P2, dOc, t2, l);    // dV^T[d][kv] += dO^T[d][q] P[q][kv]
      acc_second_stage_half_r<T, HD, 1>(dK, dS2, Qc, t2, l);    // dK^T[d][kv] += Q^T[d][q] dS[q][kv]
    }
    }
    if (nxt < end) lstore(rstore, cur ^ 1);
    __syncthreads();
    cur ^= 1;
    it = nxt; nxt = nxt2; nxt2 = nxt2 < end ? next_item(nxt2 + 1) : end;
  };
  while (it < end) {
    step(R0, R1);
    if (it >= end) break;
    step(R1, R0);
  }
  const int pos = p.rope_pos ? p.rope_pos[tok0 + min(kv, p.T - 1)] : min(kv, p.T - 1);
  T* Os = Qs;
#pragma unroll
  for (int j = 0; j < HD / 16; ++j) dK[0][j] *= scale;
  store_grad_tile<T, HD>(dK[0], true, p.rope_cos, p.rope_sin, pos, Os, w, l);
  __syncthreads();
  copy_out_tile<T, HD>(Os, (T*)p.dk + (tok0 + kvt * 64) * p.ldg + kvh * HD, p.ldg, kvt * 64, p.T, t, p.f8_amax ? p.f8_amax + 1 : nullptr);
  __syncthreads();
  store_grad_tile<T, HD>(dV[0], false, p.rope_cos, p.rope_sin, pos, Os, w, l);
  __syncthreads();
  copy_out_tile<T, HD>(Os, (T*)p.dv + (tok0 + kvt * 64) * p.ldg + kvh * HD, p.ldg, kvt * 64, p.T, t, p.f8_amax ? p.f8_amax + 2 : nullptr);
}


// -DATTN_KV_TRACE (tools/trace_attn_kv.sh; never in the product build): wave 0 of every attn_bwd_kv32_kernel workgroup stamps the wall
// clock (10 ns) at entry, after the first item is staged, after the item loop and at exit, and sums the item loop's phases -- issue of the
// next item's DMA and scalar loads, arithmetic, publishing (waits for the DMA), barrier.  rsys_attn_trace_read copies the table out.
#ifdef ATTN_KV_TRACE
__device__ unsigned long long rsys_attn_trace[16 * 8192];
#define KVT_NOW() ((unsigned long long)wall_clock64())
#else
#define KVT_NOW() 0ull
#endif

// ------------------------------------------------------------------------ dK, dV on v_mfma_f32_32x32x16_bf16 (bf16, head_dim 64)
// The item loops above are bound by instruction ISSUE (profiles/r4_pmc_attention_sq.txt: the waves' active cycles add up to the SIMDs'
// issue capacity; an MFMA holds the vector issue port for 8 cycles whatever its shape).  This kernel does the same arithmetic with half
// the MFMA instructions, half the LDS fragment reads and half the staging per FLOP: a wave owns 32 keys (the lanes' l & 31) and runs
// 32 x 32 x 16 products, four waves = 128 keys = two kv tiles per workgroup, each staged Q / dO tile feeds all of them.
//   S[q][kv] = sum_d Q[q][d] K[kv][d]:  A = Q rows from LDS (ds_read_b128: row q0 + (l & 31), d = 16 s + 8 (l >> 5) ..+7), B = K from registers
//   dV^T[d][kv] += dO^T[d][q] P[q][kv]: the P accumulator registers 8 s .. 8 s + 7 ARE the B operand of k-step s (rows 16 s + 8 (j >> 2) +
//   4 (l >> 5) + (j & 3)); the matching A operand is read transposed from the row-major tile (two ds_read_b64_tr_b16: rows R .. R + 3 and R + 8 ..)
// LDS image: unpadded 128-byte rows, 16-byte chunk c of row r in slot c ^ sw32(r), sw32(r) = (r1, r2, r3) as bits (2, 1, 0): with that
// permutation the 32-row ds_read_b128 fragments (lane groups {0-3, 12-15, 20-27}, ...) and the 4-row x 4-chunk transposed reads of a
// 32-lane half both touch every bank once (checked against the guide's lane groups; the 16-row kernels' c ^ (r & 7) is 2-way here).
static bool attn_kv_pairs(const AttnParams& p) { return p.hd == 64 && p.is_bf16 && attn_dma_on(); }
#ifndef ATTN_KV32_WPS
#define ATTN_KV32_WPS 3   // waves per SIMD the kernel is compiled for: 168 registers, 5 dwords spilled OUTSIDE the item loop; 2 (189 registers) is 9 % slower (profiles/r5_ab_attn_kv32.log)
#endif
template <int LG>
__global__ __launch_bounds__(256, ATTN_KV32_WPS) void attn_bwd_kv32_kernel(AttnParams p) {
  [[maybe_unused]] unsigned long long tr_[12] = {KVT_NOW(), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // (-DATTN_KV_TRACE only: tools/trace_attn_kv.sh)
  constexpr int HD = 64, TB = 64 * 64;   // elements of an unpadded tile
  using T = bf16;
  using W = typename AMap<LG>::W;
  constexpr int NTM = 1 << LG;   // item = head of the group * NTM + q tile
  const W *kmap = map_ptr<LG>(p.kmap), *kmap_full = map_ptr<LG>(p.kmap_full), *kmap16 = map_ptr<LG>(p.kmap16);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  unsigned char* const Qb = smem_raw;                   // [2][64 q][128 B] swizzled
  unsigned char* const dOb = smem_raw + 2 * TB * 2;     // [2][64 q][128 B]
  float* const lse2 = (float*)(smem_raw + 4 * TB * 2);  // [2][64]
  float* const dls = lse2 + 128;                        // [2][64]
  const int rep = p.H / p.KV, nt = (p.T + 63) / 64, npair = (nt + 1) / 2;
  int grp, pr;
  attn_work(p.B * p.KV, npair, p.order_k, grp, pr);
  const int b = grp / p.KV, kvh = grp % p.KV;
  const int t = threadIdx.x, l = t & 63, r32 = l & 31, h = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int kvt = 2 * pr + (w >> 1);                    // this wave's kv tile (may be nt: the odd tile's partner does nothing)
  const bool tile_ok = kvt < nt;
  const long long tok0 = (long long)b * p.T;
  const float scale = rsqrtf((float)HD), c2 = scale * LOG2E;
  const int kv = kvt * 64 + 32 * (w & 1) + r32;        // this lane's key/value token
  bf16x8 kf[4], vf[4];
  {
    const int kr = min(kv, p.T - 1);
    const T* krow = (const T*)p.k + (tok0 + kr) * p.ld + kvh * HD;
    const T* vrow = (const T*)p.v + (tok0 + kr) * p.ld + kvh * HD;
#pragma unroll
    for (int s = 0; s < 4; ++s) { kf[s] = *(const bf16x8*)(krow + 16 * s + 8 * h); vf[s] = *(const bf16x8*)(vrow + 16 * s + 8 * h); }
  }
  f32x16 dK[2], dV[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) { dK[0][i] = 0.f; dK[1][i] = 0.f; dV[0][i] = 0.f; dV[1][i] = 0.f; }
  const int qa = p.q_active != nullptr ? p.q_active[b] : NTM;
  const W act = map_below<LG>(qa);
  const int t0i = b * nt + 2 * pr, t1i = min(2 * pr + 1, nt - 1) + b * nt;
  const W bits = map_uniform((W)((kmap[t0i] | (2 * pr + 1 < nt ? kmap[t1i] : (W)0)) & act));   // q tiles the workgroup stages (union of its two kv tiles)
  const int kti = b * nt + min(kvt, nt - 1);
  const W fullbits = tile_ok ? map_uniform(kmap_full[kti]) : (W)0;
  const W wbits = tile_ok ? map_uniform((W)(kmap16[kti * 4 + 2 * (w & 1)] | kmap16[kti * 4 + 2 * (w & 1) + 1])) : (W)0;
  const at_i32x4 q_rs = at_rsrc((const T*)p.q + tok0 * p.ld + kvh * rep * HD, ((long long)(p.T - 1) * p.ld + rep * HD) * sizeof(T));
  const at_i32x4 do_rs = at_rsrc((const T*)p.dO + tok0 * p.ldo + kvh * rep * HD, ((long long)(p.T - 1) * p.ldo + rep * HD) * sizeof(T));
  const at_i32x4 lse_rs = at_rsrc(p.lse + ((long long)b * p.H + kvh * rep) * p.T, (long long)rep * p.T * 4);
  const at_i32x4 dl_rs = at_rsrc(p.delta + ((long long)b * p.H + kvh * rep) * p.T, (long long)rep * p.T * 4);
  // the pair bits of this wave's kv tile against every q tile: [nt][64 keys] words (an absent tile: an empty window, all zero)
  const at_i32x4 kb_rs = at_rsrc(p.kbits + (long long)kti * nt * 64, tile_ok ? (long long)nt * 64 * 8 : 0);
  // wave w fills rows 16 w .. 16 w + 15 of each tile with two DMA instructions (8 rows = 1 KB each): per-lane source offsets, fixed
  int qv_[2], dv_[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int row = 16 * w + 8 * k + (l >> 3), ch = (l & 7) ^ sw32(row);
    qv_[k] = (int)((row * p.ld + ch * 8) * sizeof(T));
    dv_[k] = (int)((row * p.ldo + ch * 8) * sizeof(T));
  }
  // fragment addresses inside a tile (bytes; lane constants, the item / block / k-step parts are immediates):
  //   row reads: row q0 + r32, chunk 2 s + h -> slot (2 s) ^ G, G = h ^ sw32(r32)
  //   transposed reads: row q0 + 16 s2 + 8 u + 4 h + (i >> 2), columns 32 db + 16 g16 + 4 (i & 3) -> slot L ^ (4 db) ^ u
  const int G = h ^ sw32(r32);
  const int i16 = l & 15, g16 = (l >> 4) & 1;
  const int Lc = (2 * g16 + ((i16 & 3) >> 1)) ^ ((((i16 >> 2) >> 1) & 1) << 2 | (h << 1));
  int a_row[4], a_tr[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) a_row[s] = r32 * 128 + (((2 * s) ^ G) << 4);
#pragma unroll
  for (int v = 0; v < 4; ++v) a_tr[v] = (4 * h + (i16 >> 2)) * 128 + ((Lc ^ ((v >> 1) << 2) ^ (v & 1)) << 4) + ((i16 & 1) << 3);   // v = 2 db + u
  const bool w0 = w == 0;
  const unsigned int lds0 = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(unsigned long long)(LDS_AS unsigned char*)smem_raw);
  int sx = 0, sy = 0; unsigned long long skb = 0ull;   // the next item's row scalars (wave 0) and this lane's pair-bit word on their way
  auto stage = [&](int it, int buf) {   // it = head-in-group * NTM + q tile
    const int hh = it >> LG, qt = it & (NTM - 1);
    const int qso = (int)((qt * 64 * p.ld + hh * HD) * sizeof(T)), dso = (int)((qt * 64 * p.ldo + hh * HD) * sizeof(T));
    const unsigned int qd = lds0 + buf * (TB * 2) + (16 * w) * 128, dd = qd + 2 * TB * 2;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      dma16_asm(q_rs, qd + k * 1024, qv_[k], qso);
      dma16_asm(do_rs, dd + k * 1024, dv_[k], dso);
    }
    skb = __builtin_bit_cast(unsigned long long, rsys_at_buffer_load_b64(kb_rs, 8 * (32 * (w & 1) + r32), qt * 512, 0));
    if (w0) {
      const int so = (hh * p.T + qt * 64) * 4;
      sx = rsys_at_buffer_load_b32(lse_rs, 4 * l, so, 0);
      sy = rsys_at_buffer_load_b32(dl_rs, 4 * l, so, 0);
    }
  };
  auto publish = [&](int buf) {   // the scalars into LDS; every DMA of this wave landed
    // -lse / scale: what the S chains start from, so that p = exp2(c2 * S') needs no subtraction (1 / scale = 8 is exact); -delta likewise for dP
    if (w0) { lse2[buf * 64 + l] = __builtin_bit_cast(float, sx) * -8.0f; ((int*)dls)[buf * 64 + l] = sy ^ 0x80000000; }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };
  // items = (head of the group, q tile in `bits`), heads outermost: a scalar iterator, two scalar instructions per step
  const int end = rep * NTM;
  auto next_item = [&](int from) {
    int hh = from >> LG, qt = from & (NTM - 1);
    while (hh < rep) {
      const int n = next_bit(bits, qt);
      if (n < nt) return hh * NTM + n;
      ++hh; qt = 0;
    }
    return end;
  };
  int it = next_item(0), cur = 0;
  unsigned long long wk = 0ull;
  if (it < end) { stage(it, 0); publish(0); wk = skb; }
  // The K / V fragments' loads are retired HERE, in the compiler's own bookkeeping: left pending into the loop, its wait-count pass
  // keeps counted vmcnt waits in front of the loop's first MFMAs on every trip, and those counts do not know about the LDS-DMA issued
  // behind asm just before them -- vector memory retires in order, so each such wait would drain the DMA of the NEXT item
  // (s_waitcnt vmcnt(8) .. (1) in the ISA of the first build: the arithmetic of an item began by waiting for the next item's tiles).
#pragma unroll
  for (int s = 0; s < 4; ++s) asm volatile("" : "+v"(kf[s]), "+v"(vf[s]));
  asm volatile("" : "+v"(wk));
  __syncthreads();
  tr_[1] = KVT_NOW();
  while (it < end) {
    [[maybe_unused]] const unsigned long long ta = KVT_NOW();
    const int nxt = next_item(it + 1);
    if (nxt < end) stage(nxt, cur ^ 1);   // (the other buffer: every wave left it before the barrier that ended the previous item)
    [[maybe_unused]] const unsigned long long tb = KVT_NOW();
    if ((wbits >> (it & (NTM - 1))) & 1u) {
      const bool fullt = (fullbits >> (it & (NTM - 1))) & 1u;
      const unsigned char* Qc = Qb + cur * (TB * 2);
      const unsigned char* dOc = dOb + cur * (TB * 2);
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {   // 32 queries at a time
        f32x16 S, dP;
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // accumulator rows 4 k .. 4 k + 3 = queries 32 qb + 8 k + 4 h ..+3
          const float4 l4 = *(const float4*)(lse2 + cur * 64 + 32 * qb + 8 * k + 4 * h);
          const float4 d4 = *(const float4*)(dls + cur * 64 + 32 * qb + 8 * k + 4 * h);
          S[4 * k] = l4.x; S[4 * k + 1] = l4.y; S[4 * k + 2] = l4.z; S[4 * k + 3] = l4.w;       // the S chain starts from -lse[q] / scale
          dP[4 * k] = d4.x; dP[4 * k + 1] = d4.y; dP[4 * k + 2] = d4.z; dP[4 * k + 3] = d4.w;   // the dP chain starts from -delta[q]
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          S = mfma32(*(const bf16x8*)(Qc + qb * 4096 + a_row[s]), kf[s], S);       // S[q][kv]
          dP = mfma32(*(const bf16x8*)(dOc + qb * 4096 + a_row[s]), vf[s], dP);    // dP[q][kv] - delta[q]
        }
        // bit (query) of the lane's key word: query 32 qb + 8 (r >> 2) + 4 h + (r & 3).  A 32 x 32 block of which every pair is allowed
        // needs no mask (wave-uniform: one compare and a ballot): with ~5 % of the events carrying a token-mask id a 64 x 64 tile is
        // rarely full, a block of 32 keys often is
        const unsigned int w32 = (unsigned int)(qb ? (wk >> 32) : wk);
        if (!fullt && __builtin_amdgcn_ballot_w64(w32 != 0xFFFFFFFFu) != 0ull) {
          const int src = (int)(w32 >> (4 * h));
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m = __builtin_amdgcn_sbfe(src, 8 * (r >> 2) + (r & 3), 1);
            const float sv = S[r];
            S[r] = __builtin_bit_cast(float, (__builtin_bit_cast(int, sv) & m) | (__builtin_bit_cast(int, -1e30f) & ~m));
          }
        }
        f32x16 P, dS;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pv = fexp2(S[r] * c2);   // = exp(q.k / sqrt(hd) - lse); masked: exp2(-1.8e29) = 0
          P[r] = pv;
          dS[r] = pv * dP[r];   // (the 1/sqrt(hd) factor of dS is applied once to dK at the end)
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {   // k-step = 16 queries: accumulator registers 8 s2 .. 8 s2 + 7
          const bf16x8 pf = pack8f(P, 8 * s2), sf = pack8f(dS, 8 * s2);
#pragma unroll
          for (int db = 0; db < 2; ++db) {
            const int o = (32 * qb + 16 * s2) * 128;
            const bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_AS bf16x4*)(dOc + o + a_tr[2 * db]));
            const bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_AS bf16x4*)(dOc + o + 8 * 128 + a_tr[2 * db + 1]));
            dV[db] = mfma32(__builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7), pf, dV[db]);   // dV^T[d][kv] += dO^T[d][q] P[q][kv]
            const bf16x4 q0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_AS bf16x4*)(Qc + o + a_tr[2 * db]));
            const bf16x4 q1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LDS_AS bf16x4*)(Qc + o + 8 * 128 + a_tr[2 * db + 1]));
            dK[db] = mfma32(__builtin_shufflevector(q0, q1, 0, 1, 2, 3, 4, 5, 6, 7), sf, dK[db]);   // dK^T[d][kv] += Q^T[d][q] dS[q][kv]
          }
        }
      }
    }
#ifdef ATTN_KV_TRACE
    asm volatile("" ::"v"(dK[0][0]), "v"(dV[0][0]));
    const unsigned long long tc = KVT_NOW();
#endif
    if (nxt < end) publish(cur ^ 1);
    [[maybe_unused]] const unsigned long long td = KVT_NOW();
    __syncthreads();
#ifdef ATTN_KV_TRACE
    const unsigned long long te = KVT_NOW();
    tr_[4] += tb - ta; tr_[5] += tc - tb; tr_[6] += td - tc; tr_[7] += te - td; tr_[8] += 1; tr_[9] += (wbits >> (it & (NTM - 1))) & 1u;
#endif
    wk = skb;
    cur ^= 1;
    it = nxt;
  }
  tr_[2] = KVT_NOW();
  // epilogue: dK (scaled, un-rotated) and dV as bf16 rows [key][64] through the two Q buffers (128 keys x 128 bytes each), then row stores.
  // accumulator register r of block db: d = 32 db + 8 (r >> 2) + 4 h + (r & 3), key = r32 of this wave
  const int pos = p.rope_pos ? p.rope_pos[tok0 + min(kv, p.T - 1)] : min(kv, p.T - 1);
  unsigned char* const Ks_ = Qb;                 // [128 keys][128 B]: wave w's keys at rows 32 w ..
  unsigned char* const Vs_ = Qb + 128 * 128;
  const int orow = 32 * w + r32;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d = 32 * db + 8 * g4 + 4 * h;
      float o[4] = {dK[db][4 * g4] * scale, dK[db][4 * g4 + 1] * scale, dK[db][4 * g4 + 2] * scale, dK[db][4 * g4 + 3] * scale};
      const float2 cc = *(const float2*)(p.rope_cos + pos * 32 + (d >> 1));
      const float2 ss = *(const float2*)(p.rope_sin + pos * 32 + (d >> 1));
      const float a0 = o[0] * cc.x + o[1] * ss.x, a1 = -o[0] * ss.x + o[1] * cc.x;
      const float b0 = o[2] * cc.y + o[3] * ss.y, b1 = -o[2] * ss.y + o[3] * cc.y;
      bf16x4 ko; ko[0] = (bf16)a0; ko[1] = (bf16)a1; ko[2] = (bf16)b0; ko[3] = (bf16)b1;
      bf16x4 vo; vo[0] = (bf16)dV[db][4 * g4]; vo[1] = (bf16)dV[db][4 * g4 + 1]; vo[2] = (bf16)dV[db][4 * g4 + 2]; vo[3] = (bf16)dV[db][4 * g4 + 3];
      // (chunk slot permuted by the row so that the 8-byte stores of a half-wave spread over the banks; the copy below undoes it)
      const int off = orow * 128 + ((((d >> 3) ^ (orow & 7)) << 4) | ((d & 4) << 1));
      *(bf16x4*)(Ks_ + off) = ko;
      *(bf16x4*)(Vs_ + off) = vo;
    }
  __syncthreads();
  {
    float amk = 0.f, amv = 0.f;
#pragma unroll
    for (int c = t; c < 128 * 8; c += 256) {   // 16-byte chunks of the 128 rows
      const int row = c >> 3, ch = c & 7;
      const int tile = 2 * pr + (row >> 6), key = tile * 64 + (row & 63);
      if (tile < nt && key < p.T) {
        const int off = row * 128 + ((ch ^ (row & 7)) << 4);
        const uint4 kq = *(const uint4*)(Ks_ + off), vq = *(const uint4*)(Vs_ + off);
        *(uint4*)((T*)p.dk + (tok0 + key) * p.ldg + kvh * HD + ch * 8) = kq;
        *(uint4*)((T*)p.dv + (tok0 + key) * p.ldg + kvh * HD + ch * 8) = vq;
        if (p.f8_amax != nullptr) { amk = fmaxf(amk, chunk_amax<bf16>(kq)); amv = fmaxf(amv, chunk_amax<bf16>(vq)); }
      }
    }
    if (p.f8_amax != nullptr) {
      amk = wave_max(amk); amv = wave_max(amv);
      if (l == 0) { f8_amax_add(p.f8_amax + 1, amk); f8_amax_add(p.f8_amax + 2, amv); }
    }
  }
#ifdef ATTN_KV_TRACE
  tr_[3] = KVT_NOW();
  if (threadIdx.x == 0 && blockIdx.x < 8192) for (int i = 0; i < 12; ++i) rsys_attn_trace[blockIdx.x * 16 + i] = tr_[i];
#endif
}

// ------------------------------------------------------------------------ backward: dQ (one workgroup per q tile and R heads of a kv group)
template <typename T, int HD, int R, bool DMA = false, int LG = 5>
#ifndef ATTN_DQ_WPS
#define ATTN_DQ_WPS 3   // waves per SIMD the two-head LDS-DMA form is compiled for (4: 128 registers, 13 spilled dwords; A/B in profiles/r4_ab_attn_dq_four_waves.log)
#endif
__global__ __launch_bounds__(256, (is_bf16<T>::value && HD <= 64) ? (R == 1 ? 3 : (DMA ? ATTN_DQ_WPS : 2)) : 1) void attn_bwd_q_kernel(AttnParams p) {
  using C = ACfg<T, HD>;
  using M = AMma<T>;
  using W = typename AMap<LG>::W;
  static_assert(!DMA || (is_bf16<T>::value && HD == 64), "LDS-DMA staging: bf16, head_dim 64");
  constexpr int TILE = DMA ? 64 * 64 : C::TILE;   // elements of a staged tile (DMA: unpadded, swizzled; attn_fwd_kernel)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* Ks = (T*)smem_raw;                  // [2][64 kv][LDD]
  T* Vs = Ks + 2 * TILE;                 // [2][64 kv][LDD]
  unsigned long long* ab = (unsigned long long*)(Vs + 2 * TILE);   // [2][64] pair bits of the 64 queries against the staged tile's keys
  const int nt = (p.T + 63) / 64;
  int grp, inner;
  attn_work(p.B * p.KV, (p.H / p.KV / R) * nt, p.order_q, grp, inner);
  const int b = grp / p.KV, kvh = grp % p.KV, h0 = kvh * (p.H / p.KV) + (inner / nt) * R, qt = inner % nt;
  const int t = threadIdx.x, l = t & 63, w = t >> 6, g = l >> 4, fr = l & 15;
  const long long tok0 = (long long)b * p.T;
  if (p.q_active != nullptr && qt >= p.q_active[b]) {   // dO of these queries is identically zero: so is dQ (uniform: whole workgroup)
    constexpr int CPRZ = HD / C::E;
    for (int c = t; c < 64 * CPRZ * R; c += 256) {
      const int r = c / (64 * CPRZ), cc = c % (64 * CPRZ), row = cc / CPRZ, ch = cc % CPRZ;
      if (qt * 64 + row < p.T) *(uint4*)((T*)p.dq + (tok0 + qt * 64 + row) * p.ldg + (h0 + r) * HD + ch * C::E) = make_uint4(0, 0, 0, 0);
    }
    return;
  }
  const float scale = rsqrtf((float)HD), c2 = scale * LOG2E;
  const int q = qt * 64 + w * 16 + fr;
  const bool qv = q < p.T;
  typename M::Frag qf[R][C::NDS], dof[R][C::NDS];
  float dl[R], lse2[R];
  f32x4 dQ[R][HD / 16];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int h = h0 + r;
    const T* qrow = (const T*)p.q + (tok0 + min(q, p.T - 1)) * p.ld + h * HD;
    const T* drow = (const T*)p.dO + (tok0 + min(q, p.T - 1)) * p.ldo + h * HD;
#pragma unroll
    for (int s = 0; s < C::NDS; ++s) { qf[r][s] = frag_global<T>(qrow, s * C::KS, HD, l); dof[r][s] = frag_global<T>(drow, s * C::KS, HD, l); }
    const long long so = ((long long)b * p.H + h) * p.T + min(q, p.T - 1);
    // delta = rowsum(dO * O) of this lane's query: the four lanes that share a query hold disjoint quarters of d in their
    // fragments.  Written out for the dK/dV kernel, which runs after this one.
    float d_ = 0.f;
    const T* orow = (const T*)p.o + (tok0 + min(q, p.T - 1)) * p.ldo + h * HD;
#pragma unroll
    for (int s = 0; s < C::NDS; ++s) d_ += frag_dot(dof[r][s], frag_global<T>(orow, s * C::KS, HD, l));
    d_ += __shfl_xor(d_, 16, 64);
    d_ += __shfl_xor(d_, 32, 64);
    if (!qv) d_ = 0.f;
    if (g == 0 && qv) p.delta[so] = d_;
    dl[r] = d_;
    lse2[r] = qv ? p.lse[so] * LOG2E : 0.f;
#pragma unroll
    for (int j = 0; j < HD / 16; ++j) dQ[r][j] = f32x4{0, 0, 0, 0};
  }
  if constexpr (!DMA) for (int i = 0; i < 2; ++i) { zero_pad_cols<T, HD>(Ks + i * C::TILE, t); zero_pad_cols<T, HD>(Vs + i * C::TILE, t); }
  // (scalars through readfirstlane: loaded by vector memory -- the maps are not const -- and otherwise still pending when the item loop begins)
  const W bits = map_uniform(map_ptr<LG>(p.qmap)[b * nt + qt]), fullbits = map_uniform(map_ptr<LG>(p.qmap_full)[b * nt + qt]);
  const W wbits = map_uniform(map_ptr<LG>(p.qmap16)[(b * nt + qt) * 4 + w]);
  // K / V of this kv head, rows of this sequence ([T][HD] windows of the row-major qkv), and the rows' uid / tm (tile_load_buf)
  const at_i32x4 k_rs = at_rsrc((const T*)p.k + tok0 * p.ld + kvh * HD, ((long long)(p.T - 1) * p.ld + HD) * sizeof(T));
  const at_i32x4 v_rs = at_rsrc((const T*)p.v + tok0 * p.ld + kvh * HD, ((long long)(p.T - 1) * p.ld + HD) * sizeof(T));
  // the pair bits of this q tile against every kv tile: [nt][64 queries] words (AttnParams::qbits)
  const at_i32x4 qb_rs = at_rsrc(p.qbits + ((long long)b * nt + qt) * nt * 64, (long long)nt * 64 * 8);
  TileOffs<T, HD> kv_of;
  tile_offsets<T, HD>(kv_of, p.ld, t);
  const bool w0 = __builtin_amdgcn_readfirstlane(w) == 0;
  TileRegs<T, HD> rk, rv;
  unsigned long long rb = 0ull;
  int dv_[2] = {0, 0};   // DMA: per-lane source offsets of the wave's two instructions per tile (attn_fwd_kernel)
  if constexpr (DMA) {
#pragma unroll
    for (int k = 0; k < 2; ++k) { const int row = 16 * w + 8 * k + (l >> 3); dv_[k] = (int)((row * p.ld + ((l & 7) ^ (row & 7)) * 8) * sizeof(T)); }
  }
  auto gload = [&](int kt, int buf) {
    const int so = (int)(kt * 64 * p.ld * sizeof(T));
    if constexpr (DMA) {
      unsigned char* kd = (unsigned char*)(Ks + buf * TILE) + (16 * w) * 128;
      unsigned char* vd = (unsigned char*)(Vs + buf * TILE) + (16 * w) * 128;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        dma16<ATTN_QSIDE_DMA_ASM>(k_rs, kd + k * 1024, dv_[k], so);
        dma16<ATTN_QSIDE_DMA_ASM>(v_rs, vd + k * 1024, dv_[k], so);
      }
    } else {
      tile_load_buf<T, HD>(rk, k_rs, kv_of, so);
      tile_load_buf<T, HD>(rv, v_rs, kv_of, so);
    }
    if (w0) rb = __builtin_bit_cast(unsigned long long, rsys_at_buffer_load_b64(qb_rs, 8 * l, kt * 512, 0));   // query l's keys of tile kt
  };
  auto lstore = [&](int buf) {
    if constexpr (!DMA) {
      tile_store<T, HD>(rk, Ks + buf * TILE, t);
      tile_store<T, HD>(rv, Vs + buf * TILE, t);
    }
    if (w0) ab[buf * 64 + l] = rb;
    if constexpr (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };
  int kt = next_bit(bits, 0), cur = 0;
  if (kt < nt) { gload(kt, 0); lstore(0); }
  if constexpr (DMA && ATTN_QSIDE_DMA_ASM) {   // retire the Q / dO fragments' and row scalars' loads before the loop (see dma16)
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int s = 0; s < C::NDS; ++s) asm volatile("" : "+v"(qf[r][s]), "+v"(dof[r][s]));
      asm volatile("" : "+v"(dl[r]), "+v"(lse2[r]));
    }
  }
  __syncthreads();
  while (kt < nt) {
    const int nxt = next_bit(bits, kt + 1);
    if (nxt < nt) gload(nxt, cur ^ 1);
    const T* Kc = Ks + cur * TILE;
    const T* Vc = Vs + cur * TILE;
    if ((wbits >> kt) & 1u) {
    const bool partial = !((fullbits >> kt) & 1u);
    const unsigned long long wq = ab[cur * 64 + w * 16 + fr] >> (4 * g);   // the lane's query against the tile's 64 keys (mask_bits_block)
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {   // 32 keys at a time: both stages, two score blocks per head alive
      f32x4 dS[R][2];
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
        const int i = 2 * t2 + ii;
        f32x4 S[R], dP[R];
        const f32x4 s0 = partial ? mask_bias_block(wq, i) : f32x4{0, 0, 0, 0};   // the mask as the chains' starting value, one for every head
#pragma unroll
        for (int r = 0; r < R; ++r) { S[r] = s0; dP[r] = f32x4{-dl[r], -dl[r], -dl[r], -dl[r]}; }
        first_stage_block_r<T, HD, R, DMA>(S, Kc, qf, i, l);      // S^T[kv][q] (+ mask)
        first_stage_block_r<T, HD, R, DMA>(dP, Vc, dof, i, l);    // dP^T[kv][q] - delta[q]
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const float pv = fexp2(fmaf(S[r][rr], c2, -lse2[r]));
            dS[r][ii][rr] = pv * dP[r][rr];   // (the 1/sqrt(hd) factor of dS is applied once to dQ at the end)
          }
      }
      acc_second_stage_half_r<T, HD, R, DMA>(dQ, dS, Kc, t2, l);    // dQ^T[d][q] += K^T[d][kv] dS^T[kv][q]
    }
    }
    if (nxt < nt) lstore(cur ^ 1);
    __syncthreads();
    cur ^= 1;
    kt = nxt;
  }
  const int pos = p.rope_pos ? p.rope_pos[tok0 + min(q, p.T - 1)] : min(q, p.T - 1);
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int j = 0; j < HD / 16; ++j) dQ[r][j] *= scale;
    store_grad_tile<T, HD>(dQ[r], true, p.rope_cos, p.rope_sin, pos, Ks + r * C::TILE, w, l);   // (head r in the r-th staged-tile slot)
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < R; ++r)
    copy_out_tile<T, HD>(Ks + r * C::TILE, (T*)p.dq + (tok0 + qt * 64) * p.ldg + (h0 + r) * HD, p.ldg, qt * 64, p.T, t, p.f8_amax);
}

template <typename T, int HD, int LG>
static int attn_bwd_hd(const AttnParams& p, hipStream_t s) {
  using C = ACfg<T, HD>;
  const size_t sm_kv = sizeof(T) * 4 * C::TILE + 512 * 4;
  const size_t sm_q = sizeof(T) * 4 * C::TILE + 384 * 4;
  static bool set = false;
  if (!set) {
    HIP_CHECK(hipFuncSetAttribute((const void*)attn_bwd_kv_kernel<T, HD, LG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm_kv));
    HIP_CHECK(hipFuncSetAttribute((const void*)attn_bwd_q_kernel<T, HD, 1, false, LG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm_q));
    HIP_CHECK(hipFuncSetAttribute((const void*)attn_bwd_q_kernel<T, HD, 2, false, LG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm_q));
    set = true;
  }
  // the dQ kernel also produces delta = rowsum(dO * O), which the dK/dV kernel reads
  bool q_done = false;
  if constexpr (is_bf16<T>::value && HD == 64) {
    if (attn_dma_on()) {
      const size_t sm_dma = 4 * 64 * 64 * 2 + 384 * 4;
      if (attn_heads_per_wg(p) == 2) hipLaunchKernelGGL((attn_bwd_q_kernel<T, HD, 2, true, LG>), dim3(((p.T + 63) / 64) * (p.H / 2) * p.B), dim3(256), sm_dma, s, p);
      else hipLaunchKernelGGL((attn_bwd_q_kernel<T, HD, 1, true, LG>), dim3(((p.T + 63) / 64) * p.H * p.B), dim3(256), sm_dma, s, p);
      q_done = true;
    }
  }
  if (!q_done) {
    if (attn_heads_per_wg(p) == 2) hipLaunchKernelGGL((attn_bwd_q_kernel<T, HD, 2, false, LG>), dim3(((p.T + 63) / 64) * (p.H / 2) * p.B), dim3(256), sm_q, s, p);
    else hipLaunchKernelGGL((attn_bwd_q_kernel<T, HD, 1, false, LG>), dim3(((p.T + 63) / 64) * p.H * p.B), dim3(256), sm_q, s, p);
  }
  HIP_CHECK(hipGetLastError());
  // (two adjacent kv tiles per workgroup -- Q / dO staging and every fragment read shared by 32 keys per wave -- measured 6 % slower:
  // 254 registers, two waves per SIMD; profiles/r4_ab_attn_dkv_two_key_tiles.log)
  if constexpr (is_bf16<T>::value && HD == 64) {
    if (attn_kv_pairs(p)) {   // 32 keys per wave on 32 x 32 x 16 products, two kv tiles per workgroup (order_k lists the pairs)
      const int npair = ((p.T + 63) / 64 + 1) / 2;
      hipLaunchKernelGGL(attn_bwd_kv32_kernel<LG>, dim3(npair * p.KV * p.B), dim3(256), 4 * 64 * 64 * 2 + 256 * 4, s, p);
      HIP_CHECK(hipGetLastError());
      return RSYS_OK;
    }
  }
  hipLaunchKernelGGL((attn_bwd_kv_kernel<T, HD, LG>), dim3(((p.T + 63) / 64) * p.KV * p.B), dim3(256), sm_kv, s, p);
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}

template <typename T>
int launch_attn_bwd(const AttnParams& p, hipStream_t s) {
  int rc = check_attn(p, sizeof(T));
  if (rc) return rc;
  ARG_CHECK(p.H / p.KV <= 8, "attention: at most 8 query heads per kv head");
  const bool wide = (p.T + 63) / 64 > 32;
  switch (p.hd) {
    case 16: return wide ? attn_bwd_hd<T, 16, 6>(p, s) : attn_bwd_hd<T, 16, 5>(p, s);
    case 32: return wide ? attn_bwd_hd<T, 32, 6>(p, s) : attn_bwd_hd<T, 32, 5>(p, s);
    case 64: return wide ? attn_bwd_hd<T, 64, 6>(p, s) : attn_bwd_hd<T, 64, 5>(p, s);
    case 128: return wide ? attn_bwd_hd<T, 128, 6>(p, s) : attn_bwd_hd<T, 128, 5>(p, s);
  }
  set_error("attention: head_dim must be 16, 32, 64 or 128");
  return RSYS_ERR_ARG;
}
template int launch_attn_bwd<bf16>(const AttnParams&, hipStream_t);
template int launch_attn_bwd<float>(const AttnParams&, hipStream_t);

// ------------------------------------------------------------------------ selected-query attention (the serving compact top)
// Decode-shaped: query token sel[i] (a flat index of the [B][T] geometry; any order, duplicates allowed) against the keys of its own row in
// token order, the model's mask from uid / tm, one soft-max, H * hd outputs into COMPACT row i of `co`.  No lse.  One workgroup per (selected
// token, kv head, R query heads of it); with 1 .. 8 query rows an MFMA tile would be mostly empty, so the products are fp32 VALU dot products
// and the kernel is bound by reading the row's K | V once.  A key is spread over G = hd / E lanes (E = the elements of one 16-byte load), a
// wave takes 64 / G keys per step, and the four waves take the steps of every visited 64-key tile in turn -- tiles without an allowed pair
// for the query's tile are skipped through the token-order qmap of launch_attn_tilemap (nullptr: every tile).  Every lane keeps its own
// running (max, sum, acc[R][E]); the groups of a wave merge by lane exchanges, the waves through LDS.
template <typename T, int E> struct SelVec;
template <> struct SelVec<bf16, 8> { using V = bf16x8; };
template <> struct SelVec<float, 4> { using V = f32x4; };
template <typename T, int HD, int R>
__global__ __launch_bounds__(256) void attn_sel_kernel(AttnParams p, const int* __restrict__ sel, T* __restrict__ co, long long ldc) {
  constexpr int E = 16 / (int)sizeof(T), G = HD / E, KPW = 64 / G;
  using V = typename SelVec<T, E>::V;
  __shared__ float sm_m[4][R], sm_s[4][R];
  __shared__ float sm_acc[4][R][HD];
  const int i = blockIdx.x, g = blockIdx.y, h0 = g * (p.H / p.KV) + blockIdx.z * R;
  const int t = threadIdx.x, l = t & 63, w = t >> 6, sub = l % G, kl = l / G;
  const long long tok = sel[i];
  T* const orow = co + (long long)i * ldc + (long long)h0 * HD;
  if (tok < 0 || tok >= (long long)p.B * p.T) {   // (uniform; the callers check the list: a bad entry reads nothing and reports zeros)
    for (int c = t; c < R * HD; c += 256) orow[c] = from_f32<T>(0.f);
    return;
  }
  const int b = (int)(tok / p.T), tq = (int)(tok % p.T), nt = (p.T + 63) / 64;
  const long long base = (long long)b * p.T;
  const int uq = p.uid[tok], mq = p.tm[tok];
  const float scale = LOG2E / sqrtf((float)HD);
  float qf[R][E];
  {
    const T* qp = (const T*)p.q + tok * p.ld + (long long)h0 * HD + sub * E;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const V qv = *(const V*)(qp + r * HD);
#pragma unroll
      for (int e = 0; e < E; ++e) qf[r][e] = (float)qv[e] * scale;
    }
  }
  float mx[R], sum[R], acc[R][E];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    mx[r] = -1e30f; sum[r] = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) acc[r][e] = 0.f;
  }
  unsigned long long tiles = nt >= 64 ? ~0ull : ((1ull << nt) - 1ull);
  if (p.qmap != nullptr) {
    const int ent = b * nt + (tq >> 6);
    tiles &= nt > 32 /* 64-bit map words: attn_map_words */ ?((const unsigned long long*)p.qmap)[ent] : (unsigned long long)p.qmap[ent];
  }
  const T* const kb = (const T*)p.k + (long long)g * HD + sub * E;
  const T* const vb = (const T*)p.v + (long long)g * HD + sub * E;
  while (tiles) {   // (uniform)
    const int j = __builtin_ctzll(tiles);
    tiles &= tiles - 1ull;
    for (int c = w; c < G; c += 4) {
      const int key = j * 64 + c * KPW + kl;
      const long long row = base + (key < p.T ? key : p.T - 1);   // (a key behind the row's end: a clamped load, masked below)
      const int uk = p.uid[row], mk = p.tm[row];
      const V kv = *(const V*)(kb + row * p.ld);
      const V vv = *(const V*)(vb + row * p.ld);
      const bool ok = key < p.T && uk == uq && (mk == 0 || mk == mq);
      if (__ballot(ok) == 0ull) continue;   // (wave-uniform: none of this step's keys is allowed)
      float kf[E], vf[E];
#pragma unroll
      for (int e = 0; e < E; ++e) { kf[e] = (float)kv[e]; vf[e] = (float)vv[e]; }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e) d = fmaf(qf[r][e], kf[e], d);
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
        const float sc = ok ? d : -1e30f;
        const float mn = fmaxf(mx[r], sc);
        const float a = fexp2(mx[r] - mn), pe = ok ? fexp2(sc - mn) : 0.f;
        sum[r] = fmaf(sum[r], a, pe);
#pragma unroll
        for (int e = 0; e < E; ++e) acc[r][e] = fmaf(acc[r][e], a, pe * vf[e]);
        mx[r] = mn;
      }
    }
  }
  // the key groups of a wave -> its lanes kl == 0 (lane exchanges), then the four waves through LDS
#pragma unroll
  for (int o = G; o < 64; o <<= 1) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float mo = __shfl_xor(mx[r], o, 64), so = __shfl_xor(sum[r], o, 64);
      const float mn = fmaxf(mx[r], mo);
      const float a = fexp2(mx[r] - mn), bo = fexp2(mo - mn);
      sum[r] = sum[r] * a + so * bo;
#pragma unroll
      for (int e = 0; e < E; ++e) acc[r][e] = acc[r][e] * a + __shfl_xor(acc[r][e], o, 64) * bo;
      mx[r] = mn;
    }
  }
  if (kl == 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (sub == 0) { sm_m[w][r] = mx[r]; sm_s[w][r] = sum[r]; }
#pragma unroll
      for (int e = 0; e < E; ++e) sm_acc[w][r][sub * E + e] = acc[r][e];
    }
  }
  __syncthreads();
  for (int c = t; c < R * HD; c += 256) {
    const int r = c / HD, d = c % HD;
    float mn = sm_m[0][r];
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) mn = fmaxf(mn, sm_m[ww][r]);
    float s = 0.f, o = 0.f;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
      const float a = fexp2(sm_m[ww][r] - mn);
      s = fmaf(sm_s[ww][r], a, s);
      o = fmaf(sm_acc[ww][r][d], a, o);
    }
    orow[c] = from_f32<T>(s > 0.f ? o / s : 0.f);   // (a query always sees itself: s > 0 whenever the maps are the row's)
  }
}

template <typename T, int HD>
static int attn_sel_hd(const AttnParams& p, const int* sel, int n_sel, T* co, long long ldc, hipStream_t s) {
  const int rep = p.H / p.KV;
  const int R = rep % 8 == 0 ? 8 : rep % 4 == 0 ? 4 : rep % 2 == 0 ? 2 : 1;   // query heads of the kv head per workgroup
  const dim3 grid(n_sel, p.KV, rep / R);
  switch (R) {
    case 8: hipLaunchKernelGGL((attn_sel_kernel<T, HD, 8>), grid, dim3(256), 0, s, p, sel, co, ldc); break;
    case 4: hipLaunchKernelGGL((attn_sel_kernel<T, HD, 4>), grid, dim3(256), 0, s, p, sel, co, ldc); break;
    case 2: hipLaunchKernelGGL((attn_sel_kernel<T, HD, 2>), grid, dim3(256), 0, s, p, sel, co, ldc); break;
    default: hipLaunchKernelGGL((attn_sel_kernel<T, HD, 1>), grid, dim3(256), 0, s, p, sel, co, ldc); break;
  }
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}
template <typename T>
int launch_attn_sel(const AttnParams& p, const int* sel, int n_sel, void* c_O, long long ldc, hipStream_t s) {
  ARG_CHECK(sel != nullptr && c_O != nullptr && n_sel >= 1, "selected-query attention: a selection and its output");
  ARG_CHECK(p.B >= 1 && p.T >= 1 && (p.T + 63) / 64 <= 64, "selected-query attention: T <= 4096");
  ARG_CHECK(p.KV >= 1 && p.KV <= 65535 && p.H % p.KV == 0 && p.H / p.KV <= 65535 * 8, "selected-query attention: H % KV");
  ARG_CHECK(p.q && p.k && p.v && p.uid && p.tm, "selected-query attention: null operands");
  ARG_CHECK((p.ld * sizeof(T)) % 16 == 0 && (p.hd * sizeof(T)) % 16 == 0 && ((size_t)p.q | (size_t)p.k | (size_t)p.v) % 16 == 0,
            "selected-query attention: 16-byte row alignment");
  ARG_CHECK(ldc >= (long long)p.H * p.hd, "selected-query attention: compact rows of at least H * hd values");
  switch (p.hd) {
    case 16: return attn_sel_hd<T, 16>(p, sel, n_sel, (T*)c_O, ldc, s);
    case 32: return attn_sel_hd<T, 32>(p, sel, n_sel, (T*)c_O, ldc, s);
    case 64: return attn_sel_hd<T, 64>(p, sel, n_sel, (T*)c_O, ldc, s);
    case 128: return attn_sel_hd<T, 128>(p, sel, n_sel, (T*)c_O, ldc, s);
  }
  set_error("selected-query attention: head_dim must be 16, 32, 64 or 128");
  return RSYS_ERR_ARG;
}
template int launch_attn_sel<bf16>(const AttnParams&, const int*, int, void*, long long, hipStream_t);
template int launch_attn_sel<float>(const AttnParams&, const int*, int, void*, long long, hipStream_t);

// ------------------------------------------------------------------------ candidate attention against a cached history
// rsys_rank_cache_candidates (Finetune/embed.py:74-131 without the history half of the row).  A row holds candidates only: candidate j at
// tokens 2 j, 2 j + 1.  The key set of a query token is dense -- the 2 n_hist cached tokens of the row's slot -- plus its own pair, so
// there are no tile maps: the workgroup of a query tile walks the ceil(2 n_hist / 64) cached K / V tiles (only the last one is masked,
// where it is ragged) and then ONE "self" tile, its own 64 tokens' fresh K / V under the constant block-diagonal 2 x 2 pair mask, all
// in one online soft-max.  Fragments, staging (register-staged, double-buffered, one barrier per tile), the rounding points (P in the
// operand type, fp32 accumulation, O in the operand type) and the head grouping are attn_fwd_kernel's.  The cached tiles are read
// through a descriptor that ends at the slot's last stored row: rows past it come back as zeros, never as what an earlier user left.
// No atomics; query tiles past the row's candidates return at once and write nothing; inside the last live tile the rows of tokens
// >= 2 n_cand are written as zeros.
// The body both kernels below call: query tile qt of row b, heads h0 .. h0 + R - 1 of kv head kvh, against the nh2 cached tokens of `slot`
// and the tile's own 64 tokens; the rows of tokens >= nq (a token index of the row) are written as zeros.  Everything it is handed is
// workgroup-uniform.  Loads, the cached-tile walk, the self tile, the online soft-max, the zeroing and the stores live here, so the row
// form and the per-tile form (packed rows) have the same per-token arithmetic in the same order.
template <typename T, int HD, int R>
__device__ __forceinline__ void attn_cand_body(const CandAttnParams& p, const int b, const int kvh, const int h0, const int qt, const int nq, const int nh2,
                                               const int slot) {
  using C = ACfg<T, HD>;
  using M = AMma<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* Ks = (T*)smem_raw;                       // [2][64][LDD]
  T* Vs = Ks + 2 * C::TILE;                   // [2][64][LDD]
  const int nht = (nh2 + 63) / 64;
  const int t = threadIdx.x, l = t & 63, w = t >> 6, g = l >> 4, fr = l & 15;
  const long long tok0 = (long long)b * p.T;
  const int ldc = 2 * p.KV * HD;                             // a cached token: K of every kv head, then V
  const float c2 = rsqrtf((float)HD) * LOG2E;
  const int q = qt * 64 + w * 16 + fr;
  typename M::Frag qf[R][C::NDS];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const T* qrow = (const T*)p.qkv + (tok0 + min(q, p.T - 1)) * p.ld + (h0 + r) * HD;
#pragma unroll
    for (int s = 0; s < C::NDS; ++s) qf[r][s] = frag_global<T>(qrow, s * C::KS, HD, l);
  }
  float m_run[R], l_run[R];
  f32x4 oacc[R][HD / 16];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    m_run[r] = -1e30f; l_run[r] = 0.f;
#pragma unroll
    for (int j = 0; j < HD / 16; ++j) oacc[r][j] = f32x4{0, 0, 0, 0};
  }
  zero_pad_cols<T, HD>(Ks, t); zero_pad_cols<T, HD>(Ks + C::TILE, t);
  // the slot's cached rows [0, nh2) of this kv head (nh2 = 0: never loaded from), and the row's own fresh K / V
  const T* cbase = (const T*)p.cache + (long long)slot * p.Tc * ldc + kvh * HD;
  const long long cbytes = nh2 > 0 ? ((long long)(nh2 - 1) * ldc + HD) * sizeof(T) : 0;
  const at_i32x4 ck_rs = at_rsrc(cbase, cbytes), cv_rs = at_rsrc(cbase + p.KV * HD, cbytes);
  const long long sbytes = ((long long)(p.T - 1) * p.ld + HD) * sizeof(T);
  const at_i32x4 sk_rs = at_rsrc((const T*)p.qkv + tok0 * p.ld + (p.H + kvh) * HD, sbytes);
  const at_i32x4 sv_rs = at_rsrc((const T*)p.qkv + tok0 * p.ld + (p.H + p.KV + kvh) * HD, sbytes);
  TileOffs<T, HD> c_of, s_of;
  tile_offsets<T, HD>(c_of, ldc, t);
  tile_offsets<T, HD>(s_of, p.ld, t);
  TileRegs<T, HD> rk, rv;
  auto gload = [&](int kt) {   // tile kt < nht: cached; kt == nht: the self tile
    if (kt < nht) {
      const int so = (int)(kt * 64 * ldc * sizeof(T));
      tile_load_buf<T, HD>(rk, ck_rs, c_of, so);
      tile_load_buf<T, HD>(rv, cv_rs, c_of, so);
    } else {
      const int so = (int)(qt * 64 * p.ld * sizeof(T));
      tile_load_buf<T, HD>(rk, sk_rs, s_of, so);
      tile_load_buf<T, HD>(rv, sv_rs, s_of, so);
    }
  };
  auto lstore = [&](int buf) {
    tile_store<T, HD>(rk, Ks + buf * C::TILE, t);
    tile_store<T, HD>(rv, Vs + buf * C::TILE, t);
  };
  int cur = 0;
  gload(0); lstore(0);
  __syncthreads();
  for (int kt = 0; kt <= nht; ++kt) {
    if (kt < nht) gload(kt + 1);
    const T* Kc = Ks + cur * C::TILE;
    const T* Vc = Vs + cur * C::TILE;
    f32x4 S[R][4];
    const bool self = kt == nht;
    if (self || kt * 64 + 64 > nh2) {
      // the mask enters the score chains as their starting value (0 / -1e30, as in attn_fwd_kernel): the lane's query 16 w + fr against
      // keys 16 i + 4 g + rr of the tile -- its own pair in the self tile, the stored rows in the ragged last cached tile
      f32x4 bias[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int key = 16 * i + 4 * g + rr;
          const bool ok = self ? (key >> 1) == ((16 * w + fr) >> 1) : kt * 64 + key < nh2;
          bias[i][rr] = ok ? 0.f : -1e30f;
        }
      first_stage_r<T, HD, R>(S, Kc, qf, l, bias);
    } else {
      first_stage_r<T, HD, R>(S, Kc, qf, l);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float tmax = -1e30f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) tmax = fmaxf(tmax, S[r][i][rr]);
      tmax = quad_rows_max(tmax);
      const float m_new = fmaxf(m_run[r], tmax * c2);
      const float mu_old = fmaxf(m_run[r], -1e20f), mu_new = fmaxf(m_new, -1e20f);
      const float alpha = fexp2(mu_old - mu_new);
      float psum = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const float pv = fexp2(fmaf(S[r][i][rr], c2, -mu_new));
          S[r][i][rr] = pv;
          psum += pv;
        }
      psum = quad_rows_sum(psum);
      l_run[r] = l_run[r] * alpha + psum;
      m_run[r] = m_new;
#pragma unroll
      for (int j = 0; j < HD / 16; ++j) oacc[r][j] *= alpha;
    }
    acc_second_stage_r<T, HD, R>(oacc, S, Vc, l);
    if (kt < nht) lstore(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    T* Os = Ks + r * C::TILE;
    const float inv = l_run[r] > 0.f ? 1.f / l_run[r] : 0.f;
#pragma unroll
    for (int j = 0; j < HD / 16; ++j) {
      T* dst = Os + (w * 16 + fr) * C::LDD + 16 * j + 4 * g;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) dst[rr] = from_f32<T>(q < nq ? oacc[r][j][rr] * inv : 0.f);
    }
  }
  __syncthreads();
  // the whole tile is written: the padding tokens behind the row's last candidate get ZEROS, not what an earlier forward left in O.  Their
  // K / V of the next layer sit in this tile's self tile, where live queries meet them with P = 0 -- exact only while they are finite.
#pragma unroll
  for (int r = 0; r < R; ++r)
    copy_out_tile<T, HD>(Ks + r * C::TILE, (T*)p.o + (tok0 + qt * 64) * p.ldo + (h0 + r) * HD, p.ldo, qt * 64, p.T, t);
}

template <typename T, int HD, int R>
__global__ __launch_bounds__(256, (is_bf16<T>::value && HD <= 64) ? (R == 1 ? 3 : 2) : 1) void attn_cand_kernel(CandAttnParams p) {
  const int nt = (p.T + 63) / 64, n_inner = (p.H / p.KV / R) * nt;
  const int grp = blockIdx.x / n_inner, inner = blockIdx.x % n_inner;
  const int b = grp / p.KV, kvh = grp % p.KV, h0 = kvh * (p.H / p.KV) + (inner / nt) * R, qt = inner % nt;
  const int nq = 2 * min(max(p.n_cand[b], 0), p.T / 2);     // candidate tokens of the row
  if (qt * 64 >= nq) return;                                 // (uniform: whole workgroup)
  const int nh2 = 2 * min(max(p.n_hist[b], 0), p.Tc / 2);    // cached tokens of the row's slot
  const int slot = min(max(p.slot[b], 0), p.n_slots - 1);
  attn_cand_body<T, HD, R>(p, b, kvh, h0, qt, nq, nh2, slot);
}

// Packed candidate rows (rsys_rank_cache_candidates_packed): attn_cand_kernel with the row triple replaced by a per-tile
// lookup.  tile_seg [rows][ceil(T / 64)] names the segment of every 64-token tile (-1: a dead tile, which returns before its first load and
// writes nothing); seg [n_seg][4] = (slot, n_hist, first_tile, n_cand).  A segment is a run of whole tiles of one row, so the tile's
// "self" tile is still its own 64 tokens and the segment's last tile ends at token 64 first_tile + 2 n_cand of the row.  The lookup
// depends on blockIdx alone: the compiler keeps it in scalar registers.
template <typename T, int HD, int R>
__global__ __launch_bounds__(256, (is_bf16<T>::value && HD <= 64) ? (R == 1 ? 3 : 2) : 1) void attn_cand_tiles_kernel(CandAttnParams p) {
  const int nt = (p.T + 63) / 64, n_inner = (p.H / p.KV / R) * nt;
  const int grp = blockIdx.x / n_inner, inner = blockIdx.x % n_inner;
  const int b = grp / p.KV, kvh = grp % p.KV, h0 = kvh * (p.H / p.KV) + (inner / nt) * R, qt = inner % nt;
  const int sg = p.tile_seg[b * nt + qt];
  if (sg < 0 || sg >= p.n_seg) return;                       // (uniform: whole workgroup)
  const int* d = p.seg + 4 * sg;
  const int ft = d[2];
  if (ft < 0 || ft > qt) return;
  const int nq = min(64 * ft + 2 * max(d[3], 0), p.T);       // first token of the row behind the segment's candidates
  if (qt * 64 >= nq) return;
  const int nh2 = 2 * min(max(d[1], 0), p.Tc / 2);           // cached tokens of the segment's slot
  const int slot = min(max(d[0], 0), p.n_slots - 1);
  attn_cand_body<T, HD, R>(p, b, kvh, h0, qt, nq, nh2, slot);
}

template <typename T, int HD>
static int attn_cand_hd(const CandAttnParams& p, hipStream_t s) {
  using C = ACfg<T, HD>;
  const size_t sm = sizeof(T) * 4 * C::TILE;
  static bool set[64] = {};   // (the attribute belongs to the device: once per device of this process, all four instantiations)
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !set[dev]) {
    HIP_CHECK(hipFuncSetAttribute((const void*)attn_cand_kernel<T, HD, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    HIP_CHECK(hipFuncSetAttribute((const void*)attn_cand_kernel<T, HD, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    HIP_CHECK(hipFuncSetAttribute((const void*)attn_cand_tiles_kernel<T, HD, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    HIP_CHECK(hipFuncSetAttribute((const void*)attn_cand_tiles_kernel<T, HD, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    if (dev >= 0 && dev < 64) set[dev] = true;
  }
  const int nt = (p.T + 63) / 64;
  if (p.tile_seg) {   // packed rows: the same grid, the per-tile form
    if (p.H / p.KV == 2 && HD <= 64) hipLaunchKernelGGL((attn_cand_tiles_kernel<T, HD, 2>), dim3(nt * (p.H / 2) * p.rows), dim3(256), sm, s, p);
    else hipLaunchKernelGGL((attn_cand_tiles_kernel<T, HD, 1>), dim3(nt * p.H * p.rows), dim3(256), sm, s, p);
    HIP_CHECK(hipGetLastError());
    return RSYS_OK;
  }
  if (p.H / p.KV == 2 && HD <= 64) hipLaunchKernelGGL((attn_cand_kernel<T, HD, 2>), dim3(nt * (p.H / 2) * p.rows), dim3(256), sm, s, p);   // (heads per workgroup: as attn_heads_per_wg)
  else hipLaunchKernelGGL((attn_cand_kernel<T, HD, 1>), dim3(nt * p.H * p.rows), dim3(256), sm, s, p);
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}
template <typename T>
int launch_attn_cand(const CandAttnParams& p_in, hipStream_t s) {
  CandAttnParams p = p_in;
  if (p.Tc == 0) p.Tc = p.T;
  ARG_CHECK(p.rows >= 1 && p.n_slots >= 1, "candidate attention: rows and slots");
  ARG_CHECK(p.tile_seg ? (p.seg != nullptr && p.n_seg >= 1) : (p.slot && p.n_hist && p.n_cand), "candidate attention: row arrays, or a tile map with its segment table");
  ARG_CHECK(p.Tc >= p.T && p.Tc % 8 == 0 && p.Tc <= 4096, "candidate attention: the slot stride must be a multiple of 8, >= T and <= 4096");
  ARG_CHECK(p.T % 8 == 0 && p.T <= 4096, "candidate attention: T must be a multiple of 8 and <= 4096");
  ARG_CHECK(p.H % p.KV == 0, "candidate attention: H % KV");
  ARG_CHECK((p.ld * sizeof(T)) % 16 == 0 && (p.ldo * sizeof(T)) % 16 == 0 && (p.hd * sizeof(T)) % 16 == 0, "candidate attention: 16-byte row alignment");
  ARG_CHECK((long long)p.T * p.ld * sizeof(T) < (1ll << 31), "candidate attention: a row of qkv must stay below 2 GiB");
  switch (p.hd) {
    case 16: return attn_cand_hd<T, 16>(p, s);
    case 32: return attn_cand_hd<T, 32>(p, s);
    case 64: return attn_cand_hd<T, 64>(p, s);
    case 128: return attn_cand_hd<T, 128>(p, s);
  }
  set_error("candidate attention: head_dim must be 16, 32, 64 or 128");
  return RSYS_ERR_ARG;
}
template int launch_attn_cand<bf16>(const CandAttnParams&, hipStream_t);
template int launch_attn_cand<float>(const CandAttnParams&, hipStream_t);

// K | V of the leading 2 n_hist[r] tokens of every row -> the row's cache slot, in 16-byte chunks (rsys_rank_cache_store, once per layer)
template <typename T>
__global__ __launch_bounds__(256) void rank_cache_copy_kernel(const T* __restrict__ qkv, long long ld, int kv_off, int kvw, int T_len, int T_slot, const int* __restrict__ slot,
                                                              const int* __restrict__ n_hist, int n_slots, T* __restrict__ cache) {
  const int r = blockIdx.y, sl = slot[r];
  if (sl < 0 || sl >= n_slots) return;
  const int ntok = 2 * min(max(n_hist[r], 0), T_len / 2);
  const int cpr = kvw * (int)sizeof(T) / 16;
  const long long n = (long long)ntok * cpr;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < n; c += (long long)gridDim.x * 256) {
    const long long tok = c / cpr; const int ch = (int)(c % cpr);
    const uint4 v = *(const uint4*)((const unsigned char*)(qkv + ((long long)r * T_len + tok) * ld + kv_off) + 16 * ch);
    *(uint4*)((unsigned char*)(cache + ((long long)sl * T_slot + tok) * kvw) + 16 * ch) = v;
  }
}
template <typename T>
int launch_rank_cache_copy(const T* qkv, long long ld, int kv_off, int kvw, int T_len, int T_slot, int rows, const int* slot, const int* n_hist, int n_slots, T* cache,
                           hipStream_t s) {
  ARG_CHECK(T_slot >= T_len, "ranking cache: rows longer than a slot");
  ARG_CHECK((kvw * sizeof(T)) % 16 == 0 && (kv_off * sizeof(T)) % 16 == 0 && (ld * sizeof(T)) % 16 == 0, "ranking cache: 16-byte row alignment");
  const int cpr = kvw * (int)sizeof(T) / 16;
  const int gx = (int)std::min<long long>(((long long)T_len * cpr + 255) / 256, 64);
  hipLaunchKernelGGL((rank_cache_copy_kernel<T>), dim3(gx, rows), dim3(256), 0, s, qkv, ld, kv_off, kvw, T_len, T_slot, slot, n_hist, n_slots, cache);
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}
template int launch_rank_cache_copy<bf16>(const bf16*, long long, int, int, int, int, int, const int*, const int*, int, bf16*, hipStream_t);
template int launch_rank_cache_copy<float>(const float*, long long, int, int, int, int, int, const int*, const int*, int, float*, hipStream_t);

// Packed store rows (rsys_rank_cache_store_packed): per segment descriptor seg[i] = (row, first column c0, n_hist, slot), K | V of
// tokens [2 c0, 2 c0 + 2 n_hist) of the row -> rows [0, 2 n_hist) of the slot, in 16-byte chunks; grid (chunks, segments).  A descriptor that
// does not fit the rows or the cache copies nothing.
template <typename T>
__global__ __launch_bounds__(256) void rank_cache_copy_segments_kernel(const T* __restrict__ qkv, long long ld, int kv_off, int kvw, int T_len, int T_slot, int rows,
                                                                       const int* __restrict__ seg, int n_slots, T* __restrict__ cache) {
  const int* d = seg + 4 * blockIdx.y;
  const int r = d[0], c0 = d[1], nh = d[2], sl = d[3];
  if (r < 0 || r >= rows || sl < 0 || sl >= n_slots || c0 < 0 || nh <= 0) return;
  if (2 * ((long long)c0 + nh) > T_len || 2 * (long long)nh > T_slot) return;
  const int cpr = kvw * (int)sizeof(T) / 16;
  const long long n = (long long)2 * nh * cpr;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < n; c += (long long)gridDim.x * 256) {
    const long long tok = c / cpr; const int ch = (int)(c % cpr);
    const uint4 v = *(const uint4*)((const unsigned char*)(qkv + ((long long)r * T_len + 2 * c0 + tok) * ld + kv_off) + 16 * ch);
    *(uint4*)((unsigned char*)(cache + ((long long)sl * T_slot + tok) * kvw) + 16 * ch) = v;
  }
}
template <typename T>
int launch_rank_cache_copy_segments(const T* qkv, long long ld, int kv_off, int kvw, int T_len, int T_slot, int rows, const int* seg, int n_seg, int n_slots, T* cache,
                                    hipStream_t s) {
  ARG_CHECK(T_slot >= T_len, "ranking cache: rows longer than a slot");
  ARG_CHECK(rows >= 1 && n_seg >= 1 && n_seg <= 65535 && n_slots >= 1 && seg != nullptr, "ranking cache: rows, segments and slots");
  ARG_CHECK((kvw * sizeof(T)) % 16 == 0 && (kv_off * sizeof(T)) % 16 == 0 && (ld * sizeof(T)) % 16 == 0, "ranking cache: 16-byte row alignment");
  const int cpr = kvw * (int)sizeof(T) / 16;
  const int gx = (int)std::min<long long>(((long long)T_len * cpr + 255) / 256, 64);
  hipLaunchKernelGGL((rank_cache_copy_segments_kernel<T>), dim3(gx, n_seg), dim3(256), 0, s, qkv, ld, kv_off, kvw, T_len, T_slot, rows, seg, n_slots, cache);
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}
template int launch_rank_cache_copy_segments<bf16>(const bf16*, long long, int, int, int, int, int, const int*, int, int, bf16*, hipStream_t);
template int launch_rank_cache_copy_segments<float>(const float*, long long, int, int, int, int, int, const int*, int, int, float*, hipStream_t);

}  // namespace rsys

#ifdef ATTN_KV_TRACE
extern "C" __attribute__((visibility("default"))) int rsys_attn_trace_read(void* dst, unsigned long long n) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(rsys::rsys_attn_trace), n);
}
#endif
