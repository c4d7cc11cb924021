"""CPU: the numpy side of the attention op tests (tests/_attention_np.py) checked on its own -- the float64 reference's gradients against
central differences of its own forward THROUGH a RoPE rotation written out here from transformer.model.py:182-190, the generator's tile
classes, and the error measure's behaviour on a single wrong row."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _attention_np import (allowed_pairs, allowed_rows, attn_emul_bf16, attn_ref, bf16_round, launch_orders, make_users, order_keys,  # noqa: E402
                           row_err, tile_classes, tile_maps)


def _rope(x, cos, sin, pos):
    """model.py:182-190 on x [B][T][h][hd] with table rows pos [B][T]"""
    c = cos[pos][:, :, None, :]; s = sin[pos][:, :, None, :]
    y = np.empty_like(x)
    y[..., 0::2] = x[..., 0::2] * c - x[..., 1::2] * s
    y[..., 1::2] = x[..., 0::2] * s + x[..., 1::2] * c
    return y


@pytest.mark.parametrize("q_active", [None, [1, 2]])
def test_reference_gradients_match_central_differences(q_active):
    B, T, H, KV, hd = 2, 80, 4, 2, 8
    rng = np.random.default_rng(3)
    uid, tm = make_users(B, T, 5)
    th = rng.uniform(0, 2 * np.pi, (2 * T, hd // 2))
    cos, sin = np.cos(th), np.sin(th)
    pos = rng.integers(0, 2 * T, (B, T))
    xq = rng.standard_normal((B, T, H, hd)); xk = rng.standard_normal((B, T, KV, hd)); v = rng.standard_normal((B, T, KV, hd))
    dO = rng.standard_normal((B * T, H * hd))
    live = np.ones((B, T), bool) if q_active is None else (np.arange(T)[None] // 64) < np.array(q_active)[:, None]

    def loss(xq, xk, v):
        o = attn_ref(_rope(xq, cos, sin, pos).reshape(B * T, -1), _rope(xk, cos, sin, pos).reshape(B * T, -1), v.reshape(B * T, -1),
                     uid, tm, dO, H, KV, hd)[0]
        return float((o * dO * live.reshape(-1, 1)).sum())

    _, _, gq, gk, gv = attn_ref(_rope(xq, cos, sin, pos).reshape(B * T, -1), _rope(xk, cos, sin, pos).reshape(B * T, -1),
                                v.reshape(B * T, -1), uid, tm, dO, H, KV, hd, cos, sin, pos, q_active)
    for x, g, which in ((xq, gq, 0), (xk, gk, 1), (v, gv, 2)):
        g = g.reshape(x.shape)
        for _ in range(12):
            i = tuple(int(rng.integers(0, n)) for n in x.shape)
            args = [xq, xk, v]
            h = 1e-5
            xp = x.copy(); xp[i] += h; args[which] = xp; up = loss(*args)
            xm = x.copy(); xm[i] -= h; args[which] = xm; dn = loss(*args)
            assert abs((up - dn) / (2 * h) - g[i]) <= 1e-6 * max(1.0, abs(g[i])), (which, i, (up - dn) / (2 * h), g[i])


@pytest.mark.parametrize("B,T,long_at,hi", [(2, 328, "low", False), (8, 328, "high", False), (1, 2048, "low", True), (1, 2040, "high", True)])
def test_generator_contains_every_tile_class(B, T, long_at, hi):
    uid, tm = make_users(B, T, 11, long_at)
    c = tile_classes(uid, tm)
    nt = (T + 63) // 64
    assert c["empty"] + c["partial"] + c["full"] == B * nt * nt
    assert min(c["full"], c["partial"], c["empty"], c["idle_q16"], c["idle_k16"]) >= 1, c
    assert (uid[:, -8:] == 0).all() and uid.min() >= 0 and uid.max() < 2 ** 19 and tm.min() >= 0 and tm.max() < 4096
    if hi:
        assert min(c["full_hi"], c["partial_hi"]) >= 1 and 31 in c["q_tiles"] and 31 in c["k_tiles"], c


def test_old_style_inputs_have_no_full_tile():
    """what the new generator is for: token-mask ids drawn per token at a rate of 0.15 leave no 64 x 64 pair unmasked"""
    rng = np.random.default_rng(8328 + 64)
    uid = np.ones((8, 328), np.int32); tm = (rng.random((8, 328)) < 0.15).astype(np.int32)
    assert tile_classes(uid, tm)["full"] == 0


def test_row_measure_sees_one_wrong_row_and_the_emulation_is_close():
    B, T, H, KV, hd = 1, 136, 2, 1, 16
    rng = np.random.default_rng(2)
    uid, tm = make_users(B, T, 2)
    x = [bf16_round(rng.standard_normal((B * T, n * hd))) for n in (H, KV, KV, H)]
    ref = attn_ref(x[0], x[1], x[2], uid, tm, x[3], H, KV, hd)
    emu = attn_emul_bf16(x[0], x[1], x[2], uid, tm, x[3], H, KV, hd)
    for r, e, heads in ((ref[0], emu[0], H), (ref[2], emu[2], H), (ref[3], emu[3], KV), (ref[4], emu[4], KV)):
        err = row_err(e, r, heads)[0]
        assert 1e-4 < err < 3e-2, err                    # bf16: 2^-9 per rounding, a few roundings per element
    small = np.argmin(np.abs(ref[0]).reshape(B * T, H, hd).max(-1)[:, 1])
    bad = ref[0].copy(); bad[small, hd:] *= 1.5           # one (token, head) row off by half its own size
    e, where = row_err(bad, ref[0], H)
    assert e >= 0.49 and where == (int(small), 1)
    assert np.abs(bad - ref[0]).max() / np.abs(ref[0]).max() < e   # the whole-tensor measure rates it lower
    nan = ref[0].copy(); nan[7, 3] = np.nan
    assert row_err(nan, ref[0], H) == (np.inf, (7, 0))


# ---------------------------------------------------------------- tile_maps / launch_orders (the restatement tests/test_gpu_attention_maps.py compares with)
def _flags(words, n):
    """[...] map words -> [..., n] bool, bit j last"""
    return ((words[..., None] >> np.arange(n, dtype=words.dtype)) & words.dtype.type(1)).astype(bool)


def _pair_bits(bits):
    """[B][x][y][64] uint64 -> [B][x][y][64][64] bool, bit index last"""
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8).reshape(bits.shape + (8,)), axis=-1, bitorder="little").astype(bool)


@pytest.mark.parametrize("B,T,long_at", [(2, 328, "low"), (8, 328, "high"), (1, 2048, "low"), (1, 2040, "high"), (1, 2112, "low"), (1, 4088, "high")])
def test_tile_maps_counts_equal_tile_classes(B, T, long_at):
    uid, tm = make_users(B, T, 11, long_at)
    c = tile_classes(uid, tm)
    m = tile_maps(uid, tm)
    nt = (T + 63) // 64
    assert m["qmap"].dtype == (np.uint32 if nt <= 32 else np.uint64)
    some, full = _flags(m["qmap"], nt), _flags(m["qmap_full"], nt)                       # [B][qt][kt]
    np.testing.assert_array_equal(_flags(m["kmap"], nt), some.transpose(0, 2, 1))
    np.testing.assert_array_equal(_flags(m["kmap_full"], nt), full.transpose(0, 2, 1))
    assert not (full & ~some).any()
    q16 = _flags(m["qmap16"], nt)                                                        # [B][qt][g][kt]
    k16 = _flags(m["kmap16"], nt)                                                        # [B][kt][g][qt]
    assert not (q16 & ~some[:, :, None, :]).any() and not (k16 & ~some.transpose(0, 2, 1)[:, :, None, :]).any()
    hi = (np.arange(nt)[:, None] >= 16) | (np.arange(nt)[None, :] >= 16)
    for tag, sel in (("", np.ones((nt, nt), bool)), ("_hi", hi)):
        assert int((~some & sel).sum()) == c["empty" + tag]
        assert int((some & ~full & sel).sum()) == c["partial" + tag]
        assert int((full & sel).sum()) == c["full" + tag]
        assert int((~q16 & (some & sel)[:, :, None, :]).sum()) == c["idle_q16" + tag]
        assert int((~k16 & (some & sel).transpose(0, 2, 1)[:, :, None, :]).sum()) == c["idle_k16" + tag]
    assert sorted(np.nonzero(m["qmap"].any(0))[0].tolist()) == c["q_tiles"]
    assert sorted(np.nonzero(m["kmap"].any(0))[0].tolist()) == c["k_tiles"]


@pytest.mark.parametrize("T", [72, 328])
def test_pair_bits_are_the_allowed_matrix_and_its_transpose(T):
    B = 2
    uid, tm = make_users(B, T, 4)
    tm[0, 1:40:2] = 7                                        # masked and unmasked tokens interleaved: a[q, k] != a[k, q]
    nt = (T + 63) // 64
    a = np.zeros((B, nt * 64, nt * 64), bool)
    a[:, :T, :T] = allowed_pairs(uid, tm)
    assert (a != a.transpose(0, 2, 1)).any()
    for b in range(B):
        np.testing.assert_array_equal(allowed_rows(uid, tm, b, 8, 72), a[b, 8:72, :T])
    m = tile_maps(uid, tm)
    qb, kb = _pair_bits(m["qbits"]), _pair_bits(m["kbits"])   # [B][qt][kt][q][k], [B][kt][qt][k][q]
    np.testing.assert_array_equal(qb, a.reshape(B, nt, 64, nt, 64).transpose(0, 1, 3, 2, 4))
    np.testing.assert_array_equal(kb, qb.transpose(0, 2, 1, 4, 3))


@pytest.mark.parametrize("B,T,H,KV,R,kv_pairs,q_active", [
    (2, 328, 8, 4, 2, 1, None), (2, 328, 8, 4, 2, 0, [1, 6]), (3, 328, 4, 1, 1, 0, [0, 3, 6]), (3, 264, 2, 1, 2, 1, [5, 1, 2]),
    (2, 2112, 8, 4, 2, 1, [33, 7]), (4, 72, 2, 2, 1, 0, None)])
def test_orders_are_stable_heaviest_first_permutations(B, T, H, KV, R, kv_pairs, q_active):
    uid, tm = make_users(B, T, 3, "high")
    uid[-1] = uid[0]; tm[-1] = tm[0]                          # two identical rows: equal keys across groups
    m = tile_maps(uid, tm)
    nt = (T + 63) // 64
    keys = order_keys(m["qmap"], m["kmap"], B, T, H, KV, R, kv_pairs, q_active)
    orders = launch_orders(m["qmap"], m["kmap"], B, T, H, KV, R, kv_pairs, q_active)
    lists = 8 if B * KV % 8 == 0 else 1
    for key, order, n_inner in zip(keys, orders, ((H // KV // R) * nt, (nt + 1) // 2 if kv_pairs else nt)):
        assert key.shape == order.shape == (lists, B * KV // lists * n_inner) and order.dtype == np.int32
        for k, o in zip(key, order):
            assert sorted(o.tolist()) == list(range(len(o)))
            ko = k[o]
            assert (np.diff(ko) <= 0).all()
            assert (np.diff(o)[np.diff(ko) == 0] > 0).all()   # equal keys keep index order
        assert key.min() >= 0 and key.max() <= nt
    ident = launch_orders(m["qmap"], m["kmap"], B, T, H, KV, R, kv_pairs, q_active, identity=True)
    for o in ident:
        assert (o == np.arange(o.shape[1])).all()
    if q_active is not None and lists == 1:                   # the q side follows q_active: an inactive tile has no work
        per = keys[0].reshape(B, KV, H // KV // R, nt).transpose(0, 3, 1, 2)
        inactive = np.arange(nt)[None, :] >= np.asarray(q_active)[:, None]
        assert inactive.any() and (per[inactive] == 0).all() and (per[~inactive] > 0).all()


def test_tile_maps_by_hand_one_user_unmasked():
    """one user, tm = 0, T = 72: everything allowed among the 72 tokens; the tile of tokens 64 .. 71 is ragged, so never full"""
    m = tile_maps(np.full((1, 72), 5, np.int32), np.zeros((1, 72), np.int32))
    ones, low8 = np.uint64(2 ** 64 - 1), np.uint64(0xFF)
    assert m["qmap"].dtype == np.uint32
    assert m["qmap"].tolist() == [[3, 3]] and m["kmap"].tolist() == [[3, 3]]
    assert m["qmap_full"].tolist() == [[1, 0]] and m["kmap_full"].tolist() == [[1, 0]]
    assert m["qmap16"].tolist() == [[[3, 3, 3, 3], [3, 0, 0, 0]]] and m["kmap16"].tolist() == [[[3, 3, 3, 3], [3, 0, 0, 0]]]
    first8 = np.where(np.arange(64) < 8, ones, np.uint64(0))
    for name in ("qbits", "kbits"):                           # (the relation is symmetric here)
        x = m[name][0]
        assert (x[0, 0] == ones).all() and (x[0, 1] == low8).all()
        assert (x[1, 0] == first8).all() and (x[1, 1] == np.where(np.arange(64) < 8, low8, np.uint64(0))).all()
    oq, ok = launch_orders(m["qmap"], m["kmap"], 1, 72, 2, 1, 2, 0, [1])
    assert oq.tolist() == [[0, 1]] and ok.tolist() == [[0, 1]]          # keys (2, 0) and (1, 1)
    oq, ok = launch_orders(m["qmap"], m["kmap"], 1, 72, 4, 1, 1, 1, None)
    assert oq.tolist() == [list(range(8))] and ok.tolist() == [[0]]     # four heads x two tiles, all of work 2; one pair of kv tiles


def test_tile_maps_by_hand_every_token_its_own_user():
    """T = 136, every token alone: only the diagonal; tokens 128 .. 135 are the ragged third tile"""
    T = 136
    uid = np.arange(T, dtype=np.int32)[None, :] + 9; tm = np.full((1, T), 3, np.int32)
    m = tile_maps(uid, tm)
    assert m["qmap"].tolist() == [[1, 2, 4]] and m["kmap"].tolist() == [[1, 2, 4]]
    assert not m["qmap_full"].any() and not m["kmap_full"].any()
    assert m["qmap16"].tolist() == [[[1] * 4, [2] * 4, [4, 0, 0, 0]]] and m["kmap16"].tolist() == m["qmap16"].tolist()
    diag = np.uint64(1) << np.arange(64, dtype=np.uint64)
    for name in ("qbits", "kbits"):
        x = m[name][0]
        for i in range(3):
            for j in range(3):
                want = np.zeros(64, np.uint64) if i != j else diag if i < 2 else np.where(np.arange(64) < 8, diag, np.uint64(0))
                assert (x[i, j] == want).all(), (name, i, j)
    # work per q tile 1, 1, 1; the second row of keys below: q_active = 2 leaves tile 2 without work on the q side, and kv tile 2 -- seen only
    # from the inactive q tile 2 -- without work on the k side
    kq, kk = order_keys(m["qmap"], m["kmap"], 1, T, 1, 1, 1, 0, [2])
    assert kq.tolist() == [[1, 1, 0]] and kk.tolist() == [[1, 1, 0]]
    kq, kk = order_keys(m["qmap"], m["kmap"], 1, T, 1, 1, 1, 1, [2])
    assert kk.tolist() == [[2, 0]]


def test_orders_by_hand():
    """maps given directly.  B = 1, KV = 1, four tiles: q tiles visit 1, 3, 3, 2 kv tiles; kv tiles are visited by 2, 1, 4, 2 q tiles"""
    qmap = np.array([[0b0001, 0b0111, 0b1101, 0b0101]], np.uint32)
    kmap = np.array([[0b1010, 0b0100, 0b1111, 0b0011]], np.uint32)
    oq, ok = launch_orders(qmap, kmap, 1, 256, 1, 1, 1, 0)
    assert oq.tolist() == [[1, 2, 3, 0]] and ok.tolist() == [[2, 0, 3, 1]]
    oq, ok = launch_orders(qmap, kmap, 1, 256, 2, 1, 1, 0)                 # two heads: slots 0 .. 3 head 0, 4 .. 7 head 1
    assert oq.tolist() == [[1, 2, 5, 6, 3, 7, 0, 4]]
    oq, ok = launch_orders(qmap, kmap, 1, 256, 1, 1, 1, 1)                 # pairs (0, 1) -> 0b1110: 3, (2, 3) -> 0b1111: 4
    assert ok.tolist() == [[1, 0]]
    oq, ok = launch_orders(qmap, kmap, 1, 256, 1, 1, 1, 0, [2])            # q tiles 2, 3 inactive; kmap & 0b0011 -> 1, 0, 2, 2
    assert oq.tolist() == [[1, 0, 2, 3]] and ok.tolist() == [[2, 3, 0, 1]]
    # eight groups -> eight lists, list x = group x alone; group = b * KV + kv head, so row b = group // KV
    qmap8 = np.repeat(qmap, 4, 0); kmap8 = np.repeat(kmap, 4, 0)
    qmap8[3] = qmap8[3, ::-1]
    oq, ok = launch_orders(qmap8, kmap8, 4, 256, 2, 2, 1, 0)
    assert oq.shape == (8, 4) and ok.shape == (8, 4)
    assert oq[:6].tolist() == [[1, 2, 3, 0]] * 6 and oq[6:].tolist() == [[1, 2, 0, 3]] * 2
