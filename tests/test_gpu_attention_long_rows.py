"""GPU: the attention kernels on rows of 33 .. 64 tiles (2048 < T <= 4096 tokens, max_sequence_length up to 2048), where a tile-map
entry is a 64-bit word (csrc/attention_common.hpp, AMap<6>): forward and backward through rsys_op_attention_ex against the float64 reference of
tests/_attention_np.py, with the helpers, the error measure and the bounds of tests/test_gpu_attention_parity.py (its docstring):
fp32 row error <= 1e-4, whole tensor 2e-5, lse 1e-4; bf16 e <= 2 E against attn_emul_bf16 on the same inputs and whole tensor 3e-2.

Every test first ASSERTS what its inputs contain, counted per (q tile, kv tile) pair from _attention_np.allowed_pairs: full, partial and
empty pairs in each quadrant of the old word boundary (tile 32), bit 63 in use on both sides, a row of one user (every map word all
ones), the first bit beyond the old word (33 tiles) and a ragged 34th tile.  Two heads per kv head (H = 2, KV = 1) throughout: head_dim 16
and 128 run the register-staged kernels, head_dim 64 in bf16 the LDS-DMA forward / dQ kernels and attn_bwd_kv32_kernel; one test runs
both kernel variants of the RSYS_ATTN_DMA switch at 64 tiles.

The last test guards the rows of up to 32 tiles, which keep their 32-bit map words and their launch order: two launches give the same bits.

Observed on an MI355X (every test prints its figures as lines that start with RATIO), over all cases.  bf16, e / E lowest - highest (bound 2)
with the largest E: O 0.86 - 1.13 (7.9e-3), dq 1.00 - 1.00 (4.1e-2), dk 0.85 - 1.27 (2.8e-2), dv 0.93 - 1.00 (8.5e-3).  fp32, worst row:
O 5.3e-6, dq 2.6e-5, dk 7.2e-6, dv 6.7e-6 (bound 1e-4).  lse, worst token: 1.6e-6 (fp32), 1.5e-6 (bf16) (bound 1e-4).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_np as an  # noqa: E402
import test_gpu_attention_parity as ap  # noqa: E402  (its _inputs / _reference / _launch / _compare / _same_bits)

pytestmark = pytest.mark.gpu
H, KV = 2, 1


def _pairs(uid, tm):
    """full / partial / empty (q tile, kv tile) pair counts of the rows, per quadrant of the tile-32 boundary (q side first: "hh" = both
    tiles >= 32, "hl" = q >= 32 and k < 32, "lh" = q < 32 and k >= 32, "ll"), and the non-empty tiles of each side"""
    B, T = uid.shape
    nt = (T + 63) // 64
    a = np.zeros((B, nt * 64, nt * 64), bool)
    a[:, :T, :T] = an.allowed_pairs(uid, tm)
    cnt = a.reshape(B, nt, 64, nt, 64).sum((2, 4))
    hi = np.arange(nt) >= 32
    out = {}
    for tag, qs, ks in (("hh", hi, hi), ("hl", hi, ~hi), ("lh", ~hi, hi), ("ll", ~hi, ~hi)):
        c = cnt[:, qs][:, :, ks]
        out[tag] = {"full": int((c == 4096).sum()), "partial": int(((c > 0) & (c < 4096)).sum()), "empty": int((c == 0).sum())}
    out["q_tiles"] = set(np.nonzero((cnt > 0).any((0, 2)))[0].tolist())
    out["k_tiles"] = set(np.nonzero((cnt > 0).any((0, 1)))[0].tolist())
    return out


def _check_inputs(key, T, users):
    x = ap._inputs(*key)
    c = _pairs(x["uid"], x["tm"])
    print("PAIRS", key, {k: v for k, v in c.items() if k not in ("q_tiles", "k_tiles")})
    if T == 4096 and users == "low":
        for quad in ("hh", "hl", "lh"):
            for cls in ("full", "partial", "empty"):
                assert c[quad][cls] >= 1, (quad, cls, c)
        assert 63 in c["q_tiles"] and 63 in c["k_tiles"], c
    elif T == 4096 and users == "high":
        assert c["hh"]["full"] >= 1, c
    elif T == 4096 and users == "one":
        assert all(c[quad]["empty"] == 0 for quad in ("hh", "hl", "lh", "ll")), c
    elif T == 2112:
        assert (T + 63) // 64 == 33 and c["hl"]["partial"] >= 1 and c["lh"]["partial"] >= 1, c   # partial pairs across the boundary, each side
    elif T == 2120:
        assert (T + 63) // 64 == 34 and T % 64 == 8 and c["hl"]["full"] >= 1, c


USERS = {"low": ("low", None), "high": ("high", None), "one": ("low", 4088)}
# (T, head_dim, users): B = 1 at T = 4096, B = 2 otherwise
SHAPES = [(4096, 16, "low"), (4096, 16, "high"), (4096, 16, "one"), (2112, 16, "high"), (2120, 16, "high"),
          (4096, 64, "low"), (2112, 128, "high")]


def _key(T, hd, users, dtype):
    long_at, long_len = USERS[users]
    return (1 if T == 4096 else 2, T, H, KV, hd, dtype, long_at, long_len)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("T,hd,users", SHAPES)
def test_rows_beyond_32_tiles_against_the_reference(T, hd, users, dtype):
    """O, lse, dq, dk, dv of one forward + backward launch; random-angle RoPE tables, implicit positions"""
    key = _key(T, hd, users, dtype)
    _check_inputs(key, T, users)
    rope = (T, False, None)
    ref, emu = ap._reference(key, H, KV, hd, rope, None)
    ap._compare(f"long{key}", ap._launch(key, H, KV, hd, rope), ref, emu, key, H, KV)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("qa", [40, 9])
def test_compact_top_above_and_below_the_old_word(qa, dtype):
    """q_active = 40 of 64 tiles (a mask of the active query tiles that needs the high word) and 9 (one that does not): O / lse of the active
    tiles match, dq is exactly zero beyond them, dk / dv match the reference with the inactive dO rows zeroed and stay finite although O,
    lse and delta of the inactive tiles are NaN (a kernel that reads one of them shows)."""
    T, hd = 4096, 64
    key = _key(T, hd, "low", dtype)
    _check_inputs(key, T, "low")
    rope = (T, False, None)
    live = (np.arange(T)[None, :] // 64) < qa
    dO = ap._inputs(*key)["dO"] * live.reshape(-1, 1)
    res = ap._launch(key, H, KV, hd, rope, (qa,), dO=dO, nan_out=True)
    ref, emu = ap._reference(key, H, KV, hd, rope, (qa,))
    assert not res["raw_dqkv"][~live.reshape(-1), :H * hd].any()
    assert np.isnan(res["lse"][:, :, qa * 64:]).all(), "the inactive query tiles' lse must stay untouched"
    assert np.isfinite(res["dk"]).all() and np.isfinite(res["dv"]).all()
    ap._compare(f"long-top{qa}{key}", res, ref, emu, key, H, KV, live)


def test_every_kernel_variant_on_rows_of_64_tiles(tmp_path):
    """bf16 / head_dim 64 at T = 4096 behind the RSYS_ATTN_DMA switch, as test_every_kernel_variant_on_full_tiles_and_a_real_rotation does it
    (the switch is read once per process: one fresh child per variant, one at a time, each under its own time limit; the first
    abnormal exit ends the test): the 64-bit instantiations of the register-staged forward / dQ / dK/dV kernels and of the LDS-DMA
    kernels, each against the reference; the register-staged and the LDS-DMA forward and dQ kernels run the same products in the same
    order, so O, lse and dQ must agree bit for bit."""
    T, hd = 4096, 64
    key = _key(T, hd, "low", 1)
    _check_inputs(key, T, "low")
    x = ap._inputs(*key)
    rope = (T, False, None)
    cos, sin = ap._tables(T, hd)
    src = str(tmp_path / "in.npz")
    np.savez(src, dtype=1, H=H, KV=KV, hd=hd, qkv=x["qkv"], dO=x["dO"], uid=x["uid"], tm=x["tm"], cos=cos, sin=sin,
             pos=np.arange(T, dtype=np.int32)[None, :])          # (explicit positions = the implicit ones of the reference)
    ref, emu = ap._reference(key, H, KV, hd, rope, None)
    base = {k: v for k, v in os.environ.items() if not k.startswith("RSYS_ATTN_")}
    outs = []
    for i, (name, env) in enumerate(ap.VARIANTS):
        out = str(tmp_path / f"v{i}.npz")
        subprocess.run([sys.executable, os.path.join(ap.ROOT, "tests", "_attention_worker.py"), src, out, ap.ROOT], check=True, env=dict(base, **env),
                       cwd=ap.ROOT, timeout=120)
        outs.append(dict(np.load(out)))
    for (name, _), res in zip(ap.VARIANTS, outs):
        ap._compare(f"long-variant[{name}]", res, ref, emu, key, H, KV)
    for n in ("raw_O", "lse"):
        assert ap._same_bits(outs[0][n], outs[1][n]), n
    assert ap._same_bits(outs[0]["raw_dqkv"][:, :H * hd], outs[1]["raw_dqkv"][:, :H * hd]), "dq"


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("T", [2048, 1096])
def test_rows_of_up_to_32_tiles_repeat_their_bits(T, dtype):
    """32 tiles (the last row length of the 32-bit map words) and 18 tiles with a ragged end: a second launch gives the same bits --
    the launch order and the map atomics of the narrow path are a function of the inputs alone"""
    key = (2, T, H, KV, 64, dtype, "low", None)
    rope = (T, False, None)
    a, b = ap._launch(key, H, KV, 64, rope), ap._launch(key, H, KV, 64, rope)
    for n in ("raw_O", "raw_dqkv", "lse"):
        assert ap._same_bits(a[n], b[n]), n
    assert np.isfinite(a["O"]).all() and np.isfinite(a["dq"]).all() and np.isfinite(a["dk"]).all() and np.isfinite(a["dv"]).all()
