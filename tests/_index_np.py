"""Plain NumPy restatements of the index and compaction kernels (position selection, token union, selected-first order, the row movers,
column sums and transposes): what tests/test_gpu_index_kernels.py compares the HIP kernels with, and what tests/test_index_np.py checks
on the CPU against the oracle's selection and brute-force restatements.  Loops, sorts and fancy indexing only: nothing here knows how
a kernel divides its work."""
import numpy as np


def bf16_round(x):
    """fp32 -> the fp32 value of its bf16 rounding (nearest, ties to even), by bit arithmetic"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + ((u >> 16) & 1) + 0x7FFF) & 0xFFFF0000).view(np.float32)


def bf16_bits(x):
    """fp32 -> the 16 bits of its bf16 rounding"""
    return (bf16_round(x).view(np.uint32) >> 16).astype(np.uint16)


# --------------------------------------------------------------------------------------------- selection
def select(w, topk):
    """w [N] -> (idx [topk], npos, stats [2]): positive weights in ascending index, then the others ascending, cut at topk"""
    w = np.asarray(w, np.float32).ravel()
    pos = np.flatnonzero(w > 0)
    rest = np.flatnonzero(~(w > 0))
    idx = np.concatenate([pos, rest])[:topk].astype(np.int32)
    stats = np.array([w[idx].astype(np.float64).sum(), w.astype(np.float64).sum()])
    return idx, min(pos.size, topk), stats


# --------------------------------------------------------------------------------------------- token union
def token_union(idx_lists, npos, NT):
    """idx_lists[t] (or None) with npos[t] live entries -> (tokens ascending, bits uint32 [ceil(NT / 32)], pre int32 [same], nsel);
    the token of position i of task t is 2 i + (t & 1)"""
    toks = [np.zeros(0, np.int64)]
    for t, lst in enumerate(idx_lists):
        if lst is not None:
            toks.append(2 * np.asarray(lst, np.int64)[: int(npos[t])] + (t & 1))
    toks = np.unique(np.concatenate(toks))
    assert toks.size == 0 or (toks[0] >= 0 and toks[-1] < NT)
    nw = (NT + 31) // 32
    flags = np.zeros(nw * 32, np.uint64)
    flags[toks] = 1
    bits = (flags.reshape(nw, 32) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)
    cnt = flags.reshape(nw, 32).sum(1).astype(np.int64)
    pre = (np.cumsum(cnt) - cnt).astype(np.int32)
    return toks.astype(np.int32), bits, pre, int(toks.size)


# --------------------------------------------------------------------------------------------- selected-first order
def selected_first(toks, B, T, uid, tm, rope_pos=None, identity=False):
    """toks: the selected tokens (ascending, global indices < B T).  Returns a dict of the kernel's eight outputs plus q_active.
    Inside every row the selected tokens come first in their original order, then the others in theirs (identity: nothing moves)."""
    n = B * T
    toks = np.asarray(toks, np.int64)
    slot = np.full(n, -1, np.int32)
    slot[toks] = np.arange(toks.size, dtype=np.int32)
    sel = toks.astype(np.int32)
    perm = np.empty(n, np.int32)
    q_active = np.empty(B, np.int32)
    for b in range(B):
        row = np.arange(b * T, (b + 1) * T)
        chosen = slot[row] >= 0
        perm[row] = row if identity else np.concatenate([row[chosen], row[~chosen]])
        q_active[b] = -(-T // 64) if identity else -(-int(chosen.sum()) // 64)
    pos = (np.arange(n) % T).astype(np.int32) if rope_pos is None else np.asarray(rope_pos, np.int32)
    slot_p = slot[perm]
    sel_p = np.empty(toks.size, np.int32)
    places = np.flatnonzero(slot_p >= 0)
    sel_p[slot_p[places]] = places
    return dict(slot=slot, sel=sel, perm=perm, uid_p=np.asarray(uid, np.int32)[perm], tm_p=np.asarray(tm, np.int32)[perm], pos_p=pos[perm],
                slot_p=slot_p, sel_p=sel_p, q_active=q_active)


# --------------------------------------------------------------------------------------------- row movers (values pass through unchanged)
def round_up(n, m):
    return -(-n // m) * m


def gather_rows_sel(dst, src, sel, n):
    """dst [cap][D] (pre-filled) <- rows sel[r] for r < n, zeros up to min(cap, round_up(n, 256)), the rest as it was"""
    out = dst.copy()
    out[:n] = src[sel[:n], : dst.shape[1]]
    out[n: min(dst.shape[0], round_up(n, 256))] = 0
    return out


def scatter_rows_fill(dst, src, slot_p, q_active, T):
    """dst [B T][ld] (pre-filled): place p < min(T, 64 q_active[b]) of row b <- src row slot_p, zeros where -1; columns < D only"""
    out = dst.copy()
    D = src.shape[1]
    for b in range(len(q_active)):
        for p in range(min(T, 64 * int(q_active[b]))):
            s = slot_p[b * T + p]
            out[b * T + p, :D] = src[s] if s >= 0 else 0
    return out


def scatter_rows_map(dst, src, rows):
    out = dst.copy()
    for r, m in enumerate(rows):
        out[m, : src.shape[1]] = src[r]
    return out


def gather_rows_slot(compact, slot, idx, parity):
    out = np.zeros((len(idx), compact.shape[1]), compact.dtype)
    for r, i in enumerate(idx):
        s = slot[2 * i + parity]
        if s >= 0:
            out[r] = compact[s]
    return out


def scatter_rows_add_slot(compact, src, slot, idx, parity, npos):
    out = compact.astype(np.float64)
    for r in range(min(len(idx), npos)):
        s = slot[2 * idx[r] + parity]
        if s >= 0:
            out[s] += src[r]
    return out


def gather_rows(src, idx, parity, D):
    return np.stack([src[2 * i + parity, :D] for i in idx])


def scatter_rows_add(dst, src, idx, parity, npos=None):
    out = dst.astype(np.float64)
    live = len(idx) if npos is None else min(len(idx), npos)
    for r in range(live):
        out[2 * idx[r] + parity, : src.shape[1]] += src[r]
    return out


# --------------------------------------------------------------------------------------------- column sums, casts, transposes
def colsum(src):
    """fp64 column sums and the column sums of magnitudes (what an error bound scales with)"""
    s = np.asarray(src, np.float64)
    return s.sum(0), np.abs(s).sum(0)


def cast_transpose(src, dstT):
    """dstT uint16 [D][ldt] (pre-filled) <- bf16 bits of src^T, zeros in columns [rows, round_up(rows, 64)), the rest as it was"""
    rows = src.shape[0]
    out = dstT.copy()
    out[:, :rows] = bf16_bits(src).T
    out[:, rows: round_up(rows, 64)] = 0
    return out


def transpose(dst, src, rows, cols):
    """dst [cols][ld_dst] (pre-filled) <- the transpose of src[:rows, :cols]"""
    out = dst.copy()
    out[:cols, :rows] = src[:rows, :cols].T
    return out
