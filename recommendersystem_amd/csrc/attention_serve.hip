// Attention, the serving kernels: selected-query attention of the compact top (attn_sel_kernel, launch_attn_sel) and candidate attention
// against a cached history (attn_cand_kernel / attn_cand_tiles_kernel, launch_attn_cand).  The design and the helpers shared with the
// training kernels of attention.hip: attention_common.hpp.
#include "attention_common.hpp"

namespace rsys {

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
  return attn_for_hd(p.hd, "selected-query attention", [&](auto hd) { return attn_sel_hd<T, decltype(hd)::value>(p, sel, n_sel, (T*)c_O, ldc, s); });
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
    for (int r = 0; r < R; ++r) softmax_step(m_run[r], l_run[r], oacc[r], S[r], c2);
    acc_second_stage_r<T, HD, R>(oacc, S, Vc, l);
    if (kt < nht) lstore(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }
  // the whole tile is written: the padding tokens behind the row's last candidate get ZEROS, not what an earlier forward left in O.  Their
  // K / V of the next layer sit in this tile's self tile, where live queries meet them with P = 0 -- exact only while they are finite.
  attn_o_epilogue<T, HD, R>(Ks, oacc, l_run, q < nq, (T*)p.o + (tok0 + qt * 64) * p.ldo + h0 * HD, p.ldo, qt * 64, p.T, t);
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
  const size_t sm = sizeof(T) * 4 * ACfg<T, HD>::TILE;
  int rc = attn_lds_optin<attn_cand_kernel<T, HD, 1>, attn_cand_kernel<T, HD, 2>, attn_cand_tiles_kernel<T, HD, 1>, attn_cand_tiles_kernel<T, HD, 2>>(sm);
  if (rc) return rc;
  return attn_for_form<T, HD, false>(p, [&](auto r, auto) {
    constexpr int R = decltype(r)::value;
    const dim3 grid(((p.T + 63) / 64) * (p.H / R) * p.rows);
    if (p.tile_seg) hipLaunchKernelGGL((attn_cand_tiles_kernel<T, HD, R>), grid, dim3(256), sm, s, p);   // packed rows: the same grid, the per-tile form
    else hipLaunchKernelGGL((attn_cand_kernel<T, HD, R>), grid, dim3(256), sm, s, p);
    HIP_CHECK(hipGetLastError());
    return RSYS_OK;
  });
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
  return attn_for_hd(p.hd, "candidate attention", [&](auto hd) { return attn_cand_hd<T, decltype(hd)::value>(p, s); });
}
template int launch_attn_cand<bf16>(const CandAttnParams&, hipStream_t);
template int launch_attn_cand<float>(const CandAttnParams&, hipStream_t);

}  // namespace rsys
