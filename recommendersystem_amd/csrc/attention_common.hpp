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
//
// This header: what the attention sources share -- attention_maps.hip (tile maps, launch orders), attention.hip (the training kernels),
// attention_serve.hip (selected-query and candidate attention): the device helpers, the host predicates and the launches' host helpers.
#pragma once
#include <type_traits>

#include "kernels.hpp"

namespace rsys {

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

// One online soft-max step of one head (attn_fwd_kernel, attn_cand_body): S = the lane's query against the 64 keys of a tile (masked
// entries at -1e30) -> the probabilities against the new running maximum; m_run / l_run / oacc are rescaled to it.  Log2 units: c2.
template <int NJ>
__device__ __forceinline__ void softmax_step(float& m_run, float& l_run, f32x4 (&oacc)[NJ], f32x4 (&S)[4], float c2) {
  float tmax = -1e30f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) tmax = fmaxf(tmax, S[i][rr]);
  tmax = quad_rows_max(tmax);
  const float m_new = fmaxf(m_run, tmax * c2);
  const float mu_old = fmaxf(m_run, -1e20f), mu_new = fmaxf(m_new, -1e20f);
  const float alpha = fexp2(mu_old - mu_new);
  float psum = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const float pv = fexp2(fmaf(S[i][rr], c2, -mu_new));   // masked entries: exp2(-1.8e29) = 0
      S[i][rr] = pv;
      psum += pv;
    }
  psum = quad_rows_sum(psum);
  l_run = l_run * alpha + psum;
  m_run = m_new;
#pragma unroll
  for (int j = 0; j < NJ; ++j) oacc[j] *= alpha;
}
// Their O epilogue: O^T (rows d, col q) / l_run -> row-major through LDS (head r in the r-th staged-tile slot of Ks; R <= 4: the four
// staged-tile slots), then 16-byte row stores to o = the tile's first row of head h0 (copy_out_tile).  live = false: the lane's query
// stores zeros (the candidate form's tokens behind the row's last candidate).
template <typename T, int HD, int R>
__device__ __forceinline__ void attn_o_epilogue(T* Ks, const f32x4 (&oacc)[R][HD / 16], const float (&l_run)[R], bool live, T* o, long long ldo, int tile_tok0,
                                                int T_len, int t, float* amax = nullptr) {
  using C = ACfg<T, HD>;
  const int l = t & 63, w = t >> 6, g = l >> 4, fr = l & 15;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    T* Os = Ks + r * C::TILE;   // [64][LDD]
    const float inv = l_run[r] > 0.f ? 1.f / l_run[r] : 0.f;
#pragma unroll
    for (int j = 0; j < HD / 16; ++j) {
      T* dst = Os + (w * 16 + fr) * C::LDD + 16 * j + 4 * g;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) dst[rr] = from_f32<T>(live ? oacc[r][j][rr] * inv : 0.f);
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < R; ++r) copy_out_tile<T, HD>(Ks + r * C::TILE, o + r * HD, ldo, tile_tok0, T_len, t, amax);
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

// ------------------------------------------------------------------------ host side of the launches
// query heads per workgroup of the forward / dQ / candidate kernels: the whole group of a kv head when that is 2 (every configuration of
// H / KV = 2), else 1.
inline bool attn_dma_on() { return sw().attn_dma != 0; }
template <typename P>   // (AttnParams or CandAttnParams)
inline int attn_heads_per_wg(const P& p) {
  return (p.H / p.KV == 2 && p.hd <= 64) ? 2 : 1;   // (head_dim 128: two heads' accumulators cost a wave per SIMD)
}
// the dK/dV launch of this shape is attn_bwd_kv32_kernel (order_k then lists kv tile PAIRS)
inline bool attn_kv_pairs(const AttnParams& p) { return p.hd == 64 && p.is_bf16 && attn_dma_on(); }

// One dispatch over head_dim for the four launchers: f(AInt<HD>{}) with HD = hd; `what` heads the error text of any other value.
template <int V> using AInt = std::integral_constant<int, V>;
template <typename F>
int attn_for_hd(int hd, const char* what, F&& f) {
  switch (hd) {
    case 16: return f(AInt<16>{});
    case 32: return f(AInt<32>{});
    case 64: return f(AInt<64>{});
    case 128: return f(AInt<128>{});
  }
  set_error(std::string(what) + ": head_dim must be 16, 32, 64 or 128");
  return RSYS_ERR_ARG;
}
// ... and over the map-word width: f(AInt<HD>{}, AInt<LG>{}); 64-bit map words are the AMap<6> instantiations (rows of up to 32 tiles keep the 32-bit ones)
template <typename F>
int attn_for_hd_lg(const AttnParams& p, F&& f) {
  const bool wide = (p.T + 63) / 64 > 32;
  return attn_for_hd(p.hd, "attention", [&](auto hd) { return wide ? f(hd, AInt<6>{}) : f(hd, AInt<5>{}); });
}
// The form of a kernel family K<T, HD, R, ...> at a shape: R = query heads per workgroup (attn_heads_per_wg) and, where the family has one
// (HAS_DMA; bf16 at head_dim 64 only, RSYS_ATTN_DMA=0: the register-staged kernels), LDS-DMA staging.  f(AInt<R>{}, std::bool_constant<DMA>{}).
template <typename T, int HD, bool HAS_DMA, typename P, typename F>
int attn_for_form(const P& p, F&& f) {
  const bool two = attn_heads_per_wg(p) == 2;
  if constexpr (HAS_DMA && is_bf16<T>::value && HD == 64) {
    if (attn_dma_on()) return two ? f(AInt<2>{}, std::true_type{}) : f(AInt<1>{}, std::true_type{});
  }
  return two ? f(AInt<2>{}, std::false_type{}) : f(AInt<1>{}, std::false_type{});
}
// Dynamic LDS beyond the default limit is an opt-in of a kernel that belongs to the device: once per kernel instantiations K... and device
// of this process (a per-process flag would leave the fp32 head_dim-128 kernels, 135 KB, unlaunchable on a process's second device).
template <auto... K>
int attn_lds_optin(size_t bytes) {
  static bool set[64] = {};
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !set[dev]) {
    for (const void* k : {(const void*)K...}) HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (dev >= 0 && dev < 64) set[dev] = true;
  }
  return RSYS_OK;
}

}  // namespace rsys
