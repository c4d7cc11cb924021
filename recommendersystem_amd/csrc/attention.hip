// Attention, the training kernels: forward, dQ and the two dK/dV forms, behind launch_attn_fwd / launch_attn_bwd.  The design and the
// helpers shared with attention_maps.hip (tile maps, launch orders) and attention_serve.hip (selected-query and candidate attention):
// attention_common.hpp.
#include "attention_common.hpp"

namespace rsys {

// ------------------------------------------------------------------------ the query-side K / V pipeline (forward and dQ)
// attn_fwd_kernel and attn_bwd_q_kernel walk the kv tiles of one q tile in the same way: the q tile's map words, K / V of the kv head and the
// q tile's pair bits behind buffer descriptors, gload(kt, buf) to fetch tile kt and lstore(buf) to publish it in LDS buffer buf (the kernels
// follow it with their one barrier per tile).  What differs stays in the kernels: which buffers get zero_pad_cols, and which registers the
// empty asm retires in front of the loop.
// DMA (bf16, head_dim 64): the K / V tiles arrive by LDS-DMA in unpadded XOR-swizzled tiles (frag_rows_sw).
template <typename T, int HD, bool DMA, int LG>
struct AttnKVStage {
  using W = typename AMap<LG>::W;
  static constexpr int TILE = DMA ? 64 * 64 : ACfg<T, HD>::TILE;   // elements of a staged tile
  const AttnParams& p;
  T* const Ks;                      // [2][64][LDD]   (DMA: [2][64][64] swizzled)
  T* const Vs;                      // [2][64][LDD]
  unsigned long long* const ab;     // [2][64] pair bits of the 64 queries against the staged tile's keys
  const int t, l, w;
  W bits, fullbits, wbits;          // kv tiles the q tile visits / that need no mask / that this wave's 16 queries take part in
  at_i32x4 k_rs, v_rs, qb_rs;
  TileOffs<T, HD> kv_of;
  bool w0;
  TileRegs<T, HD> rk, rv;
  unsigned long long rb = 0ull;
  int dv_[2] = {0, 0};   // DMA: wave w fills rows 16 w .. + 15 of a tile with two instructions (8 rows each); per-lane source offsets

  __device__ __forceinline__ AttnKVStage(const AttnParams& p_, unsigned char* smem, int t_)
      : p(p_), Ks((T*)smem), Vs(Ks + 2 * TILE), ab((unsigned long long*)(Vs + 2 * TILE)), t(t_), l(t_ & 63), w(t_ >> 6) {}
  // q tile qt of row b against kv head kvh (called behind the kernel's zero_pad_cols, where this text stood in both kernels)
  __device__ __forceinline__ void init(int b, int kvh, int qt) {
    const int nt = (p.T + 63) / 64;
    const long long tok0 = (long long)b * p.T;
    // (scalars through readfirstlane: loaded by vector memory -- the maps are not const -- and otherwise still pending when the item loop begins)
    bits = map_uniform(map_ptr<LG>(p.qmap)[b * nt + qt]); fullbits = map_uniform(map_ptr<LG>(p.qmap_full)[b * nt + qt]);
    wbits = map_uniform(map_ptr<LG>(p.qmap16)[(b * nt + qt) * 4 + w]);
    // K / V of this kv head, rows of this sequence ([T][HD] windows of the row-major qkv), and the rows' uid / tm (tile_load_buf)
    k_rs = at_rsrc((const T*)p.k + tok0 * p.ld + kvh * HD, ((long long)(p.T - 1) * p.ld + HD) * sizeof(T));
    v_rs = at_rsrc((const T*)p.v + tok0 * p.ld + kvh * HD, ((long long)(p.T - 1) * p.ld + HD) * sizeof(T));
    // the pair bits of this q tile against every kv tile: [nt][64 queries] words (AttnParams::qbits)
    qb_rs = at_rsrc(p.qbits + ((long long)b * nt + qt) * nt * 64, (long long)nt * 64 * 8);
    tile_offsets<T, HD>(kv_of, p.ld, t);
    w0 = __builtin_amdgcn_readfirstlane(w) == 0;
    if constexpr (DMA) {
#pragma unroll
      for (int k = 0; k < 2; ++k) { const int row = 16 * w + 8 * k + (l >> 3); dv_[k] = (int)((row * p.ld + ((l & 7) ^ (row & 7)) * 8) * sizeof(T)); }
    }
  }
  __device__ __forceinline__ void gload(int kt, int buf) {   // (DMA: straight into buffer buf; else into registers, lstore(buf) follows after the arithmetic)
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
  }
  __device__ __forceinline__ void lstore(int buf) {
    if constexpr (!DMA) {
      tile_store<T, HD>(rk, Ks + buf * TILE, t);
      tile_store<T, HD>(rv, Vs + buf * TILE, t);
    }
    if (w0) ab[buf * 64 + l] = rb;
    if constexpr (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA landed (the barrier follows)
  }
};

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
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
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
  AttnKVStage<T, HD, DMA, LG> st(p, smem_raw, t);
  constexpr int TILE = decltype(st)::TILE;
  T* const Ks = st.Ks;
  T* const Vs = st.Vs;
  if constexpr (!DMA) { zero_pad_cols<T, HD>(Ks, t); zero_pad_cols<T, HD>(Ks + C::TILE, t); }
  st.init(b, kvh, qt);
  const W bits = st.bits, fullbits = st.fullbits, wbits = st.wbits;
  int kt = next_bit(bits, 0);
  int cur = 0;
  if (kt < nt) { st.gload(kt, 0); st.lstore(0); }
  if constexpr (DMA && ATTN_QSIDE_DMA_ASM) {   // retire the Q fragments' loads in the compiler's bookkeeping before the loop (see dma16)
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int s = 0; s < C::NDS; ++s) asm volatile("" : "+v"(qf[r][s]));
  }
  __syncthreads();
  while (kt < nt) {
    const int nxt = next_bit(bits, kt + 1);
    if (nxt < nt) st.gload(nxt, cur ^ 1);
    const T* Kc = Ks + cur * TILE;
    const T* Vc = Vs + cur * TILE;
    if ((wbits >> kt) & 1u) {   // (a wave whose 16 queries have no allowed key in this tile leaves its state untouched)
    f32x4 S[R][4];
    if (!((fullbits >> kt) & 1u)) {
      // the lane's query against the tile's 64 keys (pair bits): the mask enters the score chains as their starting value
      const unsigned long long wq = st.ab[cur * 64 + w * 16 + fr] >> (4 * g);
      f32x4 bias[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) bias[i] = mask_bias_block(wq, i);
      first_stage_r<T, HD, R, DMA>(S, Kc, qf, l, bias);
    } else {
      first_stage_r<T, HD, R, DMA>(S, Kc, qf, l);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) softmax_step(m_run[r], l_run[r], oacc[r], S[r], c2);
    acc_second_stage_r<T, HD, R, DMA>(oacc, S, Vc, l);
    }
    if (nxt < nt) st.lstore(cur ^ 1);
    __syncthreads();
    cur ^= 1;
    kt = nxt;
  }
  if (g == 0 && qv) {
#pragma unroll
    for (int r = 0; r < R; ++r) p.lse[((long long)b * p.H + h0 + r) * p.T + q] = (m_run[r] + log2f(l_run[r])) * (1.f / LOG2E);
  }
  attn_o_epilogue<T, HD, R>(Ks, oacc, l_run, true, (T*)p.o + (tok0 + qt * 64) * p.ldo + h0 * HD, p.ldo, qt * 64, p.T, t, p.f8_amax);
}


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
// The dK/dV kernels' items = (head of the kv head's group, q tile in `bits`), heads outermost, numbered head << LG | q tile: the first item
// >= from, or rep << LG when they are exhausted.  A scalar iterator, two scalar instructions per step.
template <int LG>
__device__ __forceinline__ int next_kv_item(typename AMap<LG>::W bits, int from, int rep, int nt) {
  constexpr int NTM = 1 << LG;
  int hh = from >> LG, qt = from & (NTM - 1);
  while (hh < rep) {
    const int n = next_bit(bits, qt);
    if (n < nt) return hh * NTM + n;
    ++hh; qt = 0;
  }
  return rep * NTM;
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
  const int end = rep * NTM;
  auto next_item = [&](int from) { return next_kv_item<LG>(bits, from, rep, nt); };
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
  const int end = rep * NTM;
  auto next_item = [&](int from) { return next_kv_item<LG>(bits, from, rep, nt); };
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
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
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
  AttnKVStage<T, HD, DMA, LG> st(p, smem_raw, t);   // (the staged tiles: [2][64 kv][LDD] of K, then of V)
  constexpr int TILE = decltype(st)::TILE;
  T* const Ks = st.Ks;
  T* const Vs = st.Vs;
  if constexpr (!DMA) for (int i = 0; i < 2; ++i) { zero_pad_cols<T, HD>(Ks + i * C::TILE, t); zero_pad_cols<T, HD>(Vs + i * C::TILE, t); }
  st.init(b, kvh, qt);
  const W bits = st.bits, fullbits = st.fullbits, wbits = st.wbits;
  int kt = next_bit(bits, 0), cur = 0;
  if (kt < nt) { st.gload(kt, 0); st.lstore(0); }
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
    if (nxt < nt) st.gload(nxt, cur ^ 1);
    const T* Kc = Ks + cur * TILE;
    const T* Vc = Vs + cur * TILE;
    if ((wbits >> kt) & 1u) {
    const bool partial = !((fullbits >> kt) & 1u);
    const unsigned long long wq = st.ab[cur * 64 + w * 16 + fr] >> (4 * g);   // the lane's query against the tile's 64 keys (mask_bits_block)
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
    if (nxt < nt) st.lstore(cur ^ 1);
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

// ------------------------------------------------------------------------ launches
static int check_attn(const AttnParams& p, size_t esz) {
  ARG_CHECK(p.T % 8 == 0 && (p.T + 63) / 64 <= 64, "attention: T must be a multiple of 8 and <= 4096");
  ARG_CHECK(p.qbits != nullptr && p.kbits != nullptr, "attention: the pair-bit buffers (AttnParams::qbits / kbits) are required");
  ARG_CHECK(p.H % p.KV == 0, "attention: H % KV");
  ARG_CHECK((p.ld * esz) % 16 == 0 && (p.hd * esz) % 16 == 0, "attention: 16-byte row alignment");
  // (the kernels address a row's tiles through 32-bit buffer offsets: at T = 4096, ld = 4096 in bf16 a row is 32 MiB)
  ARG_CHECK((long long)p.T * std::max(p.ld, p.ldo) * (long long)esz < (1ll << 31), "attention: a row of qkv must stay below 2 GiB");
  return RSYS_OK;
}

// The two query-side families by name (a function template cannot be passed on as it is): K::get<T, HD, R, DMA, LG>() is the kernel.
struct AttnFwdK {
  template <typename T, int HD, int R, bool DMA, int LG> static constexpr auto get() { return &attn_fwd_kernel<T, HD, R, DMA, LG>; }
};
struct AttnBwdQK {
  template <typename T, int HD, int R, bool DMA, int LG> static constexpr auto get() { return &attn_bwd_q_kernel<T, HD, R, DMA, LG>; }
};
// forward and dQ: one workgroup per (q tile, R heads of a kv group), four staged tiles and the pair-bit words in LDS
template <typename K, typename T, int HD, int LG>
static int attn_qside_launch(const AttnParams& p, hipStream_t s) {
  const size_t sm = sizeof(T) * 4 * ACfg<T, HD>::TILE + 384 * 4;
  int rc = attn_lds_optin<K::template get<T, HD, 1, false, LG>(), K::template get<T, HD, 2, false, LG>()>(sm);
  if (rc) return rc;
  return attn_for_form<T, HD, true>(p, [&](auto r, auto dma) {
    constexpr int R = decltype(r)::value;
    constexpr bool DMA = decltype(dma)::value;   // (unpadded tiles: 4 * 64 * 64 * 2 + 384 * 4 bytes)
    hipLaunchKernelGGL((K::template get<T, HD, R, DMA, LG>()), dim3(((p.T + 63) / 64) * (p.H / R) * p.B), dim3(256), DMA ? (size_t)(4 * 64 * 64 * 2 + 384 * 4) : sm, s, p);
    HIP_CHECK(hipGetLastError());
    return RSYS_OK;
  });
}

template <typename T>
int launch_attn_fwd(const AttnParams& p, hipStream_t s) {
  int rc = check_attn(p, sizeof(T));
  if (rc) return rc;
  return attn_for_hd_lg(p, [&](auto hd, auto lg) { return attn_qside_launch<AttnFwdK, T, decltype(hd)::value, decltype(lg)::value>(p, s); });
}
template int launch_attn_fwd<bf16>(const AttnParams&, hipStream_t);
template int launch_attn_fwd<float>(const AttnParams&, hipStream_t);

template <typename T, int HD, int LG>
static int attn_bwd_hd(const AttnParams& p, hipStream_t s) {
  const size_t sm_kv = sizeof(T) * 4 * ACfg<T, HD>::TILE + 512 * 4;
  int rc = attn_lds_optin<attn_bwd_kv_kernel<T, HD, LG>>(sm_kv);
  if (rc) return rc;
  // the dQ kernel also produces delta = rowsum(dO * O), which the dK/dV kernel reads
  rc = attn_qside_launch<AttnBwdQK, T, HD, LG>(p, s);
  if (rc) return rc;
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
  return attn_for_hd_lg(p, [&](auto hd, auto lg) { return attn_bwd_hd<T, decltype(hd)::value, decltype(lg)::value>(p, s); });
}
template int launch_attn_bwd<bf16>(const AttnParams&, hipStream_t);
template int launch_attn_bwd<float>(const AttnParams&, hipStream_t);

}  // namespace rsys

#ifdef ATTN_KV_TRACE
extern "C" __attribute__((visibility("default"))) int rsys_attn_trace_read(void* dst, unsigned long long n) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(rsys::rsys_attn_trace), n);
}
#endif
