// Attention, before the kernels run: the tile maps and pair bits of a token order (attn_tilemap_kernel) and the heaviest-first launch
// orders (attn_order_kernel), both behind launch_attn_tilemap.  The design: attention_common.hpp.
#include "attention_common.hpp"

namespace rsys {

// token keys (uid << 12 | tm) of tokens past the end of a row: never equal to each other or to a real key (uid < 2^19)
#define KEY_NO_Q ((int)0xFFFFE000u)
#define KEY_NO_K ((int)0xFFFFFFFFu)
// allowed(q, kv) = uid equal AND (tm[kv] == 0 OR tm equal).  With the token key a = uid << 12 | tm (host-checked:
// 0 <= uid < 2^19, 0 <= tm < 4096) this is  a[kv] == (a[q] & ~4095)  OR  a[kv] == a[q].  The compares run ONCE per step and map set, in
// attn_tilemap_kernel, which keeps their outcome as pair bits (AttnParams::qbits / kbits); the attention kernels mask from those.
__device__ __forceinline__ int token_key(int uid, int tm) { return (int)(((unsigned int)uid << 12) | (unsigned int)tm); }

// ------------------------------------------------------------------------ tile maps
// qmap / qmap_full [b][q tile]: bit j = kv tile j has some / only allowed pairs; kmap* is the transposed relation; the
// *16 maps say the same per group of 16 queries (keys).  One workgroup per (row, q tile); wave w owns the tile's 16
// queries w*16 .. w*16+15 as lane-uniform values (read back from LDS), the lanes sweep the row's keys 64 at a
// time: allowed(q, kv) <=> key[kv] == key[q] or key[kv] == key[q] without its tm bits (token_key above), so a (query,
// 64 keys) step is two compares, an OR and a ballot.  Exact: "some" bits may not miss a pair, "only" bits may not claim one.
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

AttnOrderPlan attn_order_plan(const AttnParams& p) {
  AttnOrderPlan o{};
  const int nt = (p.T + 63) / 64, n_groups = p.B * p.KV;
  o.R = attn_heads_per_wg(p); o.kv_pairs = attn_kv_pairs(p) ? 1 : 0;
  o.lists = (n_groups & 7) == 0 ? 8 : 1;
  o.n_inner_q = (p.H / p.KV / o.R) * nt; o.n_inner_k = o.kv_pairs ? (nt + 1) / 2 : nt;
  // (a list beyond one workgroup's LDS: keep the plain order -- the kernels read an identity permutation)
  const int ns_max = (n_groups / o.lists) * (p.H / p.KV) * nt;
  o.chunk_cap = attn_order_chunk_cap(nt > 32 ? 6 : 5); o.chunks = (ns_max + 63) / 64;
  o.identity = o.chunks > o.chunk_cap ? 1 : 0;
  return o;
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
    const AttnOrderPlan o = attn_order_plan(p);
    const dim3 og(o.lists, 2);
    const size_t rows = (size_t)(std::min(o.chunks, o.chunk_cap) + 1);
    if (wide) hipLaunchKernelGGL(attn_order_kernel<6>, og, dim3(256), rows * 66 * 4, s, p, o.R, o.identity, o.kv_pairs);
    else hipLaunchKernelGGL(attn_order_kernel<5>, og, dim3(256), rows * 34 * 4, s, p, o.R, o.identity, o.kv_pairs);
  }
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}

}  // namespace rsys
