"""CPU: the NumPy restatements of the index and compaction kernels (tests/_index_np.py) checked against the oracle's position selection
and against brute-force O(n^2) restatements, so that the GPU tests (tests/test_gpu_index_kernels.py) compare the kernels with something
that is itself pinned; plus the invariants those tests rely on."""
import numpy as np
import pytest

import _index_np as ix
from oracle import model_np


# --------------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("N,topk,rate", [(1, 1, 1.0), (1, 1, 0.0), (37, 37, 0.3), (200, 16, 0.5), (200, 16, 0.02), (200, 1, 0.5), (513, 100, 0.0),
                                         (513, 100, 1.0)])
def test_select_is_the_oracle_selection_on_01_weights(N, topk, rate):
    rng = np.random.default_rng(N + topk)
    w = (rng.random(N) < rate).astype(np.float32)
    idx, npos, stats = ix.select(w, topk)
    assert np.array_equal(idx, model_np.select_positions(w, topk))      # overflow (#positive > topk) included
    assert npos == min(int(w.sum()), topk) and idx.size == topk
    assert stats[0] == w[idx].sum() and stats[1] == w.sum()
    assert np.all(w[idx[:npos]] > 0) and np.all(np.diff(idx[:npos]) > 0)
    if npos < topk:
        assert np.all(w[idx[npos:]] == 0) and np.all(np.diff(idx[npos:]) > 0)


def test_select_orders_by_index_not_by_weight():
    w = np.array([0, 0.25, 2, 0, 1, 0.5], np.float32)
    idx, npos, stats = ix.select(w, 5)
    assert idx.tolist() == [1, 2, 4, 5, 0] and npos == 4 and stats.tolist() == [3.75, 3.75]
    idx, npos, stats = ix.select(w, 2)
    assert idx.tolist() == [1, 2] and npos == 2 and stats.tolist() == [2.25, 3.75]


# --------------------------------------------------------------------------------------------- token union
def _union_brute(lists, npos, NT):
    toks = []
    for tok in range(NT):
        hit = False
        for t, lst in enumerate(lists):
            if lst is None:
                continue
            for r in range(npos[t]):
                hit = hit or 2 * lst[r] + (t & 1) == tok
        if hit:
            toks.append(tok)
    nw = (NT + 31) // 32
    bits, pre = [0] * nw, [0] * nw
    for tok in toks:
        bits[tok // 32] |= 1 << (tok % 32)
    for w in range(nw):
        pre[w] = sum(1 for tok in toks if tok // 32 < w)
    return toks, bits, pre


@pytest.mark.parametrize("NT,seed", [(1, 0), (31, 1), (32, 2), (33, 3), (100, 4), (130, 5)])
def test_token_union_against_brute_force(NT, seed):
    rng = np.random.default_rng(seed)
    half = [(NT + 1) // 2, NT // 2]                 # positions whose even / odd token lies inside [0, NT)
    lists, npos = [], []
    for t in range(4):
        n_max = half[t & 1]
        lst = rng.integers(0, max(n_max, 1), 12).astype(np.int32) if n_max else np.zeros(12, np.int32)
        lists.append(lst if t != 2 else None)
        npos.append(0 if (n_max == 0 or t == 3 and seed % 2) else int(rng.integers(0, 13)))
    toks, bits, pre, nsel = ix.token_union(lists, npos, NT)
    bt, bb, bp = _union_brute(lists, npos, NT)
    assert toks.tolist() == bt and bits.tolist() == bb and pre.tolist() == bp and nsel == len(bt)


def test_token_union_merges_duplicates_across_tasks_of_equal_parity():
    toks, bits, pre, nsel = ix.token_union([[3, 5, 9], [3], [5, 3, 40], None], [2, 1, 3, 0], 96)
    assert toks.tolist() == [6, 7, 10, 80] and nsel == 4
    assert bits.tolist() == [(1 << 6) | (1 << 7) | (1 << 10), 0, 1 << 16] and pre.tolist() == [0, 3, 3]


# --------------------------------------------------------------------------------------------- selected-first
def _selected_first_brute(toks, B, T, uid, tm, rope_pos, identity):
    toks = list(toks)
    n = B * T
    out = {k: [None] * n for k in ("slot", "perm", "uid_p", "tm_p", "pos_p", "slot_p")}
    out["sel"] = [None] * len(toks); out["sel_p"] = [None] * len(toks); out["q_active"] = [0] * B
    for t in range(n):
        out["slot"][t] = sum(1 for s in toks if s < t) if t in toks else -1
        if t in toks:
            out["sel"][out["slot"][t]] = t
    for b in range(B):
        n_sel = sum(1 for s in toks if b * T <= s < (b + 1) * T)
        out["q_active"][b] = (T + 63) // 64 if identity else (n_sel + 63) // 64
        for j in range(T):
            t = b * T + j
            before_sel = sum(1 for s in toks if b * T <= s < t)
            p = j if identity else (before_sel if t in toks else n_sel + (j - before_sel))
            g = b * T + p
            out["perm"][g] = t; out["uid_p"][g] = uid[t]; out["tm_p"][g] = tm[t]
            out["pos_p"][g] = j if rope_pos is None else rope_pos[t]
            out["slot_p"][g] = out["slot"][t]
            if t in toks:
                out["sel_p"][out["slot"][t]] = g
    return out


@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("B,T,rate", [(1, 8, 0.5), (3, 24, 0.3), (2, 70, 0.0), (2, 70, 1.0), (2, 130, 0.6)])
def test_selected_first_against_brute_force_and_its_invariants(B, T, rate, with_pos, identity):
    rng = np.random.default_rng(B * T + with_pos)
    n = B * T
    toks = np.flatnonzero(rng.random(n) < rate)
    uid = rng.integers(0, 1000, n); tm = rng.integers(0, 4096, n)
    rope_pos = rng.integers(0, 500, n) if with_pos else None
    got = ix.selected_first(toks, B, T, uid, tm, rope_pos, identity)
    want = _selected_first_brute(toks, B, T, uid, tm, rope_pos, identity)
    for k, v in want.items():
        assert got[k].tolist() == v, k
    # what the GPU tests rely on
    for b in range(B):
        assert sorted(got["perm"][b * T:(b + 1) * T].tolist()) == list(range(b * T, (b + 1) * T))     # a permutation of each row
    places = np.flatnonzero(got["slot_p"] >= 0)
    assert np.array_equal(got["sel_p"][got["slot_p"][places]], places)                                  # sel_p[slot_p[p]] == p
    assert np.array_equal(got["sel"][got["slot"][toks]], toks)                                          # sel[slot[t]] == t
    assert np.array_equal(got["q_active"], [-(-T // 64)] * B if identity else [-(-int(((toks // T) == b).sum()) // 64) for b in range(B)])
    if not identity:      # selected tokens lead every row, both groups in their original order
        for b in range(B):
            sp = got["slot_p"][b * T:(b + 1) * T]; k = int((sp >= 0).sum())
            assert np.all(sp[:k] >= 0) and np.all(sp[k:] < 0)
            assert np.all(np.diff(got["perm"][b * T: b * T + k]) > 0) and np.all(np.diff(got["perm"][b * T + k:(b + 1) * T]) > 0)


# --------------------------------------------------------------------------------------------- movers, sums, rounding
def test_bf16_round_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -1.0 - 2.0 ** -8, 0.0, -0.0, 3.0e38], np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, 0.0, -0.0, 3.0e38], np.float32)
    got = ix.bf16_round(x)
    assert np.array_equal(got[:7].view(np.uint32), want[:7].view(np.uint32))     # ties to even, signed zeros kept
    assert got[7].view(np.uint32) & 0xFFFF == 0 and abs(float(got[7]) - 3.0e38) <= 2.0 ** 119   # within half a bf16 ulp (2^120 in [2^127, 2^128))
    assert np.array_equal(ix.bf16_bits(x)[:2], [0x3F80, 0x3F80])


def test_movers_zero_fill_and_untouched_ranges():
    src = np.arange(600 * 4, dtype=np.float32).reshape(600, 4) + 1
    sel = np.arange(599, -1, -1)
    for n, cap in [(0, 300), (1, 300), (255, 300), (256, 300), (257, 512), (290, 300), (300, 300)]:
        out = ix.gather_rows_sel(np.full((cap, 4), -7.5, np.float32), src, sel, n)
        z = min(cap, ix.round_up(n, 256))
        assert np.array_equal(out[:n], src[sel[:n]]) and np.all(out[n:z] == 0) and np.all(out[z:] == -7.5)
    T = 72
    slot_p = np.full(2 * T, -1); slot_p[:3] = [2, 0, 1]; slot_p[T + 70] = 3
    out = ix.scatter_rows_fill(np.full((2 * T, 8), -7.5, np.float32), src[:4], slot_p, [1, 2], T)
    assert np.array_equal(out[:3, :4], src[[2, 0, 1]]) and np.all(out[3:64, :4] == 0) and np.all(out[64:T] == -7.5)
    assert np.all(out[T:T + 70, :4] == 0) and np.array_equal(out[T + 70, :4], src[3]) and np.all(out[:, 4:] == -7.5)
    slot = np.array([-1, 0, 1, -1, 2, -1])
    assert np.array_equal(ix.gather_rows_slot(src[:3], slot, [0, 1, 2], 1), [src[0], [0] * 4, [0] * 4])
    assert np.array_equal(ix.gather_rows_slot(src[:3], slot, [0, 1, 2], 0), [[0] * 4, src[1], src[2]])
    added = ix.scatter_rows_add_slot(np.ones((3, 4)), src[:3], slot, [2, 1, 0], 0, 2)
    assert np.array_equal(added, [[1] * 4, 1 + src[1], 1 + src[0]])
    added = ix.scatter_rows_add(np.ones((6, 6)), src[:3], [2, 0, 1], 1, 2)
    assert np.array_equal(added[5, :4], 1 + src[0]) and np.array_equal(added[1, :4], 1 + src[1]) and added.sum() == 36 + src[:2].sum()


def test_cast_transpose_zero_columns_and_transpose_padding():
    src = np.arange(70 * 64, dtype=np.float32).reshape(70, 64) * 0.125
    out = ix.cast_transpose(src, np.full((64, 200), 0xC0F0, np.uint16))
    assert np.array_equal(out[:, :70], ix.bf16_bits(src).T) and np.all(out[:, 70:128] == 0) and np.all(out[:, 128:] == 0xC0F0)
    m = np.arange(6 * 8, dtype=np.uint16).reshape(6, 8)
    t = ix.transpose(np.full((5, 8), 9, np.uint16), m, 6, 5)
    assert np.array_equal(t[:, :6], m[:, :5].T) and np.all(t[:, 6:] == 9)
