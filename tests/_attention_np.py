"""Plain-numpy side of the attention op tests (tests/test_gpu_attention_parity.py, tests/test_gpu_ops.py): the float64 reference of the
block-sparse masked attention forward + backward, the same computation with bf16 rounding at the kernels' rounding points, the tile-pair
classes a launch contains, the tile maps, pair bits and launch orders of a launch entry by entry (tests/test_gpu_attention_maps.py), an
input generator that produces every class, and the per-row error measure.  No GPU, no library."""
import numpy as np

TILE = 64


def bf16_round(x):
    """round to nearest even onto the bf16 grid, as the device's float -> bf16 conversion does (returned as float32)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + 0x7FFF
    return ((u + r) & 0xFFFF0000).view(np.float32)


def allowed_pairs(uid, tm):
    """[B][q][kv]: query q may see key kv <=> same user and (the key is unmasked or both carry the same mask id)"""
    return (uid[:, :, None] == uid[:, None, :]) & ((tm[:, None, :] == 0) | (tm[:, :, None] == tm[:, None, :]))


def unrotate(g, cos, sin, pos):
    """Gradient w.r.t. x of y = rope(x) given the gradient g w.r.t. y (transformer.model.py:182-190: y0 = x0 c - x1 s, y1 = x0 s + x1 c
    per interleaved pair (d, d + 1), c / s = table row pos[token], column d / 2): the transpose [c s; -s c] applied to (g0, g1).
    g [B][T][h][hd], cos / sin [rows][hd / 2], pos [B][T] int."""
    c = cos.astype(np.float64)[pos][:, :, None, :]
    s = sin.astype(np.float64)[pos][:, :, None, :]
    g0, g1 = g[..., 0::2], g[..., 1::2]
    out = np.empty_like(g)
    out[..., 0::2] = g0 * c + g1 * s
    out[..., 1::2] = -g0 * s + g1 * c
    return out


def _attention(q, k, v, uid, tm, dO, H, KV, hd, cos, sin, pos, q_active, rnd):
    B, T = uid.shape
    rep = H // KV
    # head-major [B][h][T][hd] float64, so that every product is a batched matrix product
    f = lambda a, h: np.ascontiguousarray(rnd(np.asarray(a).reshape(B, T, h, hd)).astype(np.float64).transpose(0, 2, 1, 3))
    q, k, v, dO = f(q, H), f(k, KV), f(v, KV), f(dO, H)
    if q_active is not None:        # dO of the query tiles >= q_active[b] counts as zero
        live = (np.arange(T)[None, :] // TILE) < np.asarray(q_active)[:, None]
        dO = dO * live[:, None, :, None]
    kk = np.repeat(k, rep, 1); vv = np.repeat(v, rep, 1)                      # query head h reads kv head h // rep
    sw = lambda a: a.swapaxes(-1, -2)
    back = lambda a: a.transpose(0, 2, 1, 3)                                  # -> [B][T][h][hd]
    fold = lambda a: a.reshape(B, KV, rep, T, hd).sum(2)                      # sum over the query heads of a kv head
    scale = 1.0 / np.sqrt(hd)
    s = q @ sw(kk) * scale + np.where(allowed_pairs(uid, tm), 0.0, -np.inf)[:, None]
    mx = s.max(-1, keepdims=True)
    e = np.exp(s - mx); l = e.sum(-1, keepdims=True)
    lse = (mx + np.log(l))[..., 0]
    o = rnd(rnd(e).astype(np.float64) @ vv / l).astype(np.float64)
    p = e / l
    delta = (dO * o).sum(-1, keepdims=True)                                   # [B][H][T][1], from the STORED O
    gv = back(fold(sw(rnd(p).astype(np.float64)) @ dO))
    gs = rnd(p * (dO @ sw(vv) - delta)).astype(np.float64)                    # the 1 / sqrt(hd) factor follows the products
    gq = back(gs @ kk) * scale
    gk = back(fold(sw(gs) @ q)) * scale
    o = back(o)
    if cos is not None:
        if pos is None:
            pos = np.broadcast_to(np.arange(T), (B, T))
        gq = unrotate(gq, cos, sin, np.asarray(pos).reshape(B, T)); gk = unrotate(gk, cos, sin, np.asarray(pos).reshape(B, T))
    r2 = lambda a, h: rnd(a).astype(np.float64).reshape(B * T, h * hd)
    return o.reshape(B * T, H * hd), lse, r2(gq, H), r2(gk, KV), r2(gv, KV)


def attn_ref(q, k, v, uid, tm, dO, H, KV, hd, cos=None, sin=None, pos=None, q_active=None):
    """float64 reference: masked soft-max attention forward + backward.  q [B*T][H*hd], k / v [B*T][KV*hd] arrive post-RoPE; the
    gradients are with respect to the UN-rotated q and k (unrotate above; cos = None: no rotation), v's as it is.  pos [B][T]: table
    row per token (None: the token's index in its row).  q_active [B]: dO rows of the 64-token tiles >= q_active[b] are taken as
    zero; O / lse of those rows are returned as computed but mean nothing to a caller that passes q_active.
    Returns O [B*T][H*hd], lse [B][H][T], dq [B*T][H*hd], dk, dv [B*T][KV*hd]."""
    return _attention(q, k, v, uid, tm, dO, H, KV, hd, cos, sin, pos, q_active, lambda a: a)


def attn_emul_bf16(q, k, v, uid, tm, dO, H, KV, hd, cos=None, sin=None, pos=None, q_active=None):
    """attn_ref with a bf16 rounding wherever the bf16 kernels round (csrc/attention.hip), everything between in float64 -- it says how
    much error the storage format itself produces on these inputs, nothing about summation order or the hardware exponential:
      * q, k, v, dO are bf16 (the operands of every product);
      * forward (attn_fwd_kernel): the soft-max numerators exp(s - max) are packed to bf16 for P . V (pack8 in acc_second_stage_r), the
        row sum l adds the unrounded fp32 values and divides the fp32 accumulator, O is rounded on store; the kernel rounds against
        its RUNNING maximum, this against the final one -- the same relative rounding;
      * backward: delta = rowsum(dO * O) reads the stored bf16 O (attn_bwd_q_kernel); P = exp(s - lse) is packed to bf16 for
        P^T . dO (dV: pack8 in acc_second_stage_half_r from attn_bwd_kv_kernel, pack8f in attn_bwd_kv32_kernel); dS = P (dP - delta),
        WITHOUT its 1 / sqrt(hd), is packed to bf16 for dS . K (attn_bwd_q_kernel) and dS^T . Q (the dK/dV kernels), the factor
        multiplies the fp32 accumulators; dq, dk (after the fp32 un-rotation) and dv are rounded on store (store_grad_tile and the
        epilogue of attn_bwd_kv32_kernel).
    lse has no bf16 point (fp32 scores of bf16 operands, fp32 store)."""
    return _attention(q, k, v, uid, tm, dO, H, KV, hd, cos, sin, pos, q_active, bf16_round)


def tile_classes(uid, tm):
    """What a launch on these rows contains, per (row, 64-query tile, 64-key tile) pair as attn_tilemap_kernel classifies them (a pair is
    full when all 64 x 64 token pairs are allowed: the tokens past T of a ragged last tile are allowed nothing):
    empty / partial / full pair counts; idle_q16 / idle_k16 = groups of 16 queries (keys) without an allowed pair inside a non-empty
    pair (a wave of the forward / dQ (dK/dV) kernels that skips the tile); *_hi = the same counts over the pairs whose query or key tile
    index is >= 16; q_tiles / k_tiles = the tile indices that occur in a non-empty pair as the query (key) side.
    tile_maps below is the entry-by-entry form of the same classification: the words the device must hold, not only their counts."""
    B, T = uid.shape
    nt = (T + TILE - 1) // TILE
    a = np.zeros((B, nt * TILE, nt * TILE), bool)
    a[:, :T, :T] = allowed_pairs(uid, tm)
    a = a.reshape(B, nt, TILE, nt, TILE)
    cnt = a.sum((2, 4))                                                       # [B][qt][kt]
    some = cnt > 0
    q16 = a.reshape(B, nt, 4, 16, nt, TILE).any((3, 5)).transpose(0, 1, 3, 2)          # [B][qt][kt][group]
    k16 = a.reshape(B, nt, TILE, nt, 4, 16).any((2, 5))                                 # [B][qt][kt][group]
    hi = (np.arange(nt)[:, None] >= 16) | (np.arange(nt)[None, :] >= 16)
    out = {}
    for tag, sel in (("", np.ones((nt, nt), bool)), ("_hi", hi)):
        m = sel[None]
        out["empty" + tag] = int((~some & m).sum())
        out["partial" + tag] = int((some & (cnt < TILE * TILE) & m).sum())
        out["full" + tag] = int(((cnt == TILE * TILE) & m).sum())
        out["idle_q16" + tag] = int((~q16 & (some & m)[..., None]).sum())
        out["idle_k16" + tag] = int((~k16 & (some & m)[..., None]).sum())
    out["q_tiles"] = sorted(set(np.nonzero(some.any((0, 2)))[0].tolist()))
    out["k_tiles"] = sorted(set(np.nonzero(some.any((0, 1)))[0].tolist()))
    return out


def allowed_rows(uid, tm, b, q0, q1):
    """rows q0 .. q1 - 1 of allowed_pairs(uid, tm)[b], without the [T][T] matrix"""
    return (uid[b, q0:q1, None] == uid[b, None, :]) & ((tm[b, None, :] == 0) | (tm[b, q0:q1, None] == tm[b, None, :]))


def popcount(x):
    x = np.ascontiguousarray(x)
    return np.unpackbits(x.view(np.uint8).reshape(x.shape + (x.dtype.itemsize,)), axis=-1).sum(-1).astype(np.int64)


def _bits(flags, W):
    """flags [..., n] bool -> [...] words of type W, bit j = flags[..., j]"""
    n = flags.shape[-1]
    return np.bitwise_or.reduce(flags.astype(W) << np.arange(n, dtype=W), axis=-1) if n else np.zeros(flags.shape[:-1], W)


def tile_maps(uid, tm):
    """Every word launch_attn_tilemap must write for these rows (csrc/kernels.hpp, AttnParams), from a[b, q, k] = allowed_pairs padded
    with False beyond T to nt * 64, one query tile at a time.  W = uint32 for nt <= 32 tiles, else uint64:
      qmap [B][nt] W: bit j = some pair allowed in (q tile, kv tile j); kmap [B][nt]: bit j = some pair in (q tile j, kv tile);
      qmap_full / kmap_full: the same with "all 4096 pairs" (a ragged last tile is never full);
      qmap16 [B][nt][4]: bit j = queries 16 g .. 16 g + 15 of the q tile have a pair in kv tile j;
      kmap16 [B][nt][4]: bit j = keys 16 g .. 16 g + 15 of the kv tile are seen from q tile j;
      qbits [B][qt][kt][64] uint64: bit k of word q = a[b, 64 qt + q, 64 kt + k]; kbits [B][kt][qt][64]: bit q of word k = the same pair."""
    uid = np.asarray(uid); tm = np.asarray(tm)
    B, T = uid.shape
    nt = (T + TILE - 1) // TILE
    W = np.uint32 if nt <= 32 else np.uint64
    m = {k: np.zeros((B, nt), W) for k in ("qmap", "kmap", "qmap_full", "kmap_full")}
    m["qmap16"] = np.zeros((B, nt, 4), W); m["kmap16"] = np.zeros((B, nt, 4), W)
    m["qbits"] = np.zeros((B, nt, nt, TILE), np.uint64); m["kbits"] = np.zeros((B, nt, nt, TILE), np.uint64)
    for b in range(B):
        for qt in range(nt):
            q0, q1 = qt * TILE, min(qt * TILE + TILE, T)
            a = np.zeros((TILE, nt * TILE), bool)
            a[:q1 - q0, :T] = allowed_rows(uid, tm, b, q0, q1)
            a = a.reshape(TILE, nt, TILE)                                      # [q][kt][k]
            cnt = a.sum((0, 2))
            bit = W(1) << W(qt)
            m["qmap"][b, qt] = _bits(cnt > 0, W)
            m["qmap_full"][b, qt] = _bits(cnt == TILE * TILE, W)
            m["kmap"][b] |= np.where(cnt > 0, bit, W(0))
            m["kmap_full"][b] |= np.where(cnt == TILE * TILE, bit, W(0))
            m["qmap16"][b, qt] = _bits(a.reshape(4, 16, nt, TILE).any((1, 3)), W)
            m["kmap16"][b] |= np.where(a.reshape(TILE, nt, 4, 16).any((0, 3)), bit, W(0))
            m["qbits"][b, qt] = np.ascontiguousarray(np.packbits(a.transpose(1, 0, 2), axis=-1, bitorder="little")).view("<u8")[..., 0]   # [kt][q]
            m["kbits"][b, :, qt] = np.ascontiguousarray(np.packbits(a.transpose(1, 2, 0), axis=-1, bitorder="little")).view("<u8")[..., 0]  # [kt][k]
    return m


def order_keys(qmap, kmap, B, T, H, KV, R, kv_pairs, q_active=None):
    """The work of every slot of the launch-order lists (csrc/kernels.hpp, AttnOrderPlan; attention_maps.hip, attn_order_kernel):
    (keys_q [lists][ns_q], keys_k [lists][ns_k]).  8 lists when B * KV is a multiple of 8, slot sl of list x being group (sl // n_inner) * 8 + x
    with group = b * KV + kv head; otherwise one list of all groups.  q side: n_inner = (H // KV // R) * nt, key = kv tiles the slot's q tile
    (sl % n_inner) % nt visits, 0 for a tile >= q_active[b].  k side: n_inner = nt slots of one kv tile, or (nt + 1) // 2 slots of a
    PAIR of kv tiles (kv_pairs; the second is absent when nt is odd), key = active q tiles the slot's tile(s) are visited by."""
    nt = (T + TILE - 1) // TILE
    W = qmap.dtype.type
    groups = B * KV
    lists = 8 if groups % 8 == 0 else 1
    qa = np.full(B, nt, np.int64) if q_active is None else np.asarray(q_active, np.int64)
    below = np.array([(1 << int(n)) - 1 for n in qa], dtype=W)                 # bits 0 .. q_active[b] - 1
    work_q = np.where(np.arange(nt)[None, :] < qa[:, None], popcount(qmap), 0)          # [B][nt]
    if kv_pairs:
        pad = np.concatenate([kmap, np.zeros((B, nt % 2), W)], 1).reshape(B, (nt + 1) // 2, 2)
        work_k = popcount((pad[:, :, 0] | pad[:, :, 1]) & below[:, None])
    else:
        work_k = popcount(kmap & below[:, None])
    out = []
    for work, n_inner in ((work_q, (H // KV // R) * nt), (work_k, work_k.shape[1])):
        ns = groups // lists * n_inner
        keys = np.zeros((lists, ns), np.int64)
        for x in range(lists):
            sl = np.arange(ns)
            group = (sl // n_inner) * 8 + x if lists == 8 else sl // n_inner
            keys[x] = work[group // KV, (sl % n_inner) % work.shape[1]]
        out.append(keys)
    return out[0], out[1]


def launch_orders(qmap, kmap, B, T, H, KV, R, kv_pairs, q_active=None, identity=False):
    """order_q [lists][ns_q], order_k [lists][ns_k] int32: per list the stable sort of its slots by descending work (order_keys) --
    heaviest first, equal work in slot order --, or the identity permutation where the launch takes its fallback (a list too long for
    one workgroup's table).  qmap / kmap: tile_maps' own, never the device's."""
    out = []
    for keys in order_keys(qmap, kmap, B, T, H, KV, R, kv_pairs, q_active):
        if identity:
            out.append(np.broadcast_to(np.arange(keys.shape[1], dtype=np.int32), keys.shape).copy())
        else:
            out.append(np.stack([np.argsort(-k, kind="stable") for k in keys]).astype(np.int32))
    return out[0], out[1]


def make_users(B, T, seed, long_at="low", long_len=None):
    """uid, tm [B][T] int32 with every tile class in them.  Per row: ONE long user (long_len tokens, default 0.6 (T - 8)) whose interior
    is unmasked (tm = 0: tile pairs inside it are FULL) and whose first and last 24 tokens carry mask ids from {1, 2, 4095} at a rate of
    0.3 (PARTIAL pairs); short users of 8 - 72 tokens with mask ids at 0.25 on the rest (idle 16-token groups, EMPTY pairs against the
    long user's tiles); the last 8 tokens are uid 0.  long_at: "low" = the long user starts the row, "high" = it ends at T - 8."""
    rng = np.random.default_rng(seed)
    uid = np.zeros((B, T), np.int32); tm = np.zeros((B, T), np.int32)
    ids = np.array([1, 2, 4095], np.int32)
    n = T - 8
    L = min(n, int(round(0.6 * n)) if long_len is None else long_len)
    for b in range(B):
        lo = 0 if long_at == "low" else n - L
        uid[b, lo:lo + L] = 2 ** 19 - 1 - b
        edge = np.r_[np.arange(lo, lo + min(24, L)), np.arange(lo + max(L - 24, 0), lo + L)]
        hit = edge[rng.random(edge.size) < 0.3]
        tm[b, hit] = rng.choice(ids, hit.size)
        free = np.r_[np.arange(0, lo), np.arange(lo + L, n)]
        at, user = 0, 1 + 1000 * b
        while at < free.size:
            m = int(rng.integers(8, 73))
            seg = free[at:at + m]
            uid[b, seg] = user
            tm[b, seg] = np.where(rng.random(seg.size) < 0.25, rng.choice(ids, seg.size), 0)
            at += m; user += 1
    return uid, tm


def row_err(a, b, heads, rows=None):
    """Per (token, head) row of [B*T][heads*hd] arrays: e = max_i |a_i - b_i| / max(max_i |b_i|, 1e-3 max |b|).  Returns the worst e and
    its (token row, head); rows (bool [B*T]): the token rows that count.  A NaN anywhere in a counted row of `a` gives e = inf."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    n = a.shape[0]
    a = a.reshape(n, heads, -1); b = b.reshape(n, heads, -1)
    if rows is not None:
        a, b, idx = a[rows], b[rows], np.nonzero(rows)[0]
    else:
        idx = np.arange(n)
    if a.size == 0:
        return 0.0, (-1, -1)
    d = np.abs(a - b).max(-1)
    d = np.where(np.isnan(d), np.inf, d)
    e = d / np.maximum(np.abs(b).max(-1), 1e-3 * np.abs(b).max())
    w = np.unravel_index(np.argmax(e), e.shape)
    return float(e[w]), (int(idx[w[0]]), int(w[1]))


def lse_err(a, b, rows=None):
    """Per (row, head, token) of [B][H][T]: |a - b|, NaN = inf; rows (bool [B][T]): the tokens that count.  Worst value and its (b, h, t)."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    d = np.where(np.isnan(d), np.inf, d)
    if rows is not None:
        d = np.where(rows[:, None, :], d, 0.0)
    w = np.unravel_index(np.argmax(d), d.shape)
    return float(d[w]), tuple(int(x) for x in w)
