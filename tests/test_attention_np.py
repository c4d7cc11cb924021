"""CPU: the numpy side of the attention op tests (tests/_attention_np.py) checked on its own -- the float64 reference's gradients against
central differences of its own forward THROUGH a RoPE rotation written out here from transformer.model.py:182-190, the generator's tile
classes, and the error measure's behaviour on a single wrong row."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _attention_np import attn_emul_bf16, attn_ref, bf16_round, make_users, row_err, tile_classes  # noqa: E402


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
