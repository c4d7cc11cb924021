"""GPU: the attention kernels (csrc/attention.hip) through rsys_op_attention_ex against the float64 reference of tests/_attention_np.py, on
inputs that are CHECKED to contain what each test is for: full tile pairs (the unmasked fast path of all six kernels), partial and empty
pairs, idle 16-token groups, tile indices >= 16 (bit 31 of the 32-bit tile maps included), real RoPE rotations with implicit and explicit
positions, the compact top (q_active), head_dim 128 and 4 / 8 query heads per kv head, both kernel variants of the RSYS_ATTN_DMA switch,
and the fp8 trunk's amax slots.

Error measure (row_err): per (token, head) row e = max_i |a_i - b_i| / max(max_i |b_i|, 1e-3 max |b|); the worst row is reported with its
(token row, head).  lse: per token, absolute.
  fp32: e <= 1e-4 on every row (the project's fp32 bound) and the whole-tensor max |a - b| / max |b| <= 2e-5 (lse: 1e-5).
  bf16: no number fixed in advance.  E = the worst-row error of attn_emul_bf16 (the float64 computation with bf16 rounding at the kernels'
    rounding points) against the reference on the same inputs says what the format costs; the kernel must stay within e <= 2 E per tensor
    (the factor covers summation order and the hardware exponential), and within the whole-tensor 3e-2 of the older test.  lse has no bf16
    rounding point (fp32 scores of bf16-exact operands, fp32 store), so E is zero there by construction and the fp32 bound holds in both
    modes: 1e-4 absolute per token -- fp32 sums of at most 2048 terms and an exponential / logarithm good to a few ulp on values of a few
    units give 1e-6, two orders inside.
A full pair needs one user around a whole aligned tile plus its two masked edges of 24 tokens, so rows of T = 136 and T = 72 (shapes
kept that small because they only select a head shape) cannot hold one; those cases assert the classes they can hold.

Observed on an MI355X (every test prints its figures as lines that start with RATIO).  bf16, e / E as lowest - highest over the cases of a
test group (bound 2), with the largest E of the group:
  group                      O                    dq                   dk                   dv
  a  tile classes     0.88 - 1.00 (5.8e-3)  1.00 - 1.00 (3.4e-2)  0.90 - 1.00 (1.2e-2)  1.00 - 1.00 (6.7e-3)
  b  long rows        1.00 - 1.00 (5.0e-3)  1.00 - 1.00 (2.1e-2)  1.00 - 1.02 (1.7e-2)  1.00 - 1.00 (5.8e-3)
  c  RoPE             0.95 - 1.00 (5.5e-3)  1.00 - 1.00 (2.3e-2)  1.00 - 1.00 (9.1e-3)  1.00 - 1.00 (6.2e-3)
  d  q_active         1.00 - 1.01 (5.4e-3)  1.00 - 1.00 (3.2e-2)  1.00 - 1.00 (1.4e-2)  1.00 - 1.00 (6.2e-3)
  e  head shapes      1.00 - 1.00 (5.4e-3)  1.00 - 1.00 (1.0e-1)  1.00 - 1.00 (9.2e-3)  1.00 - 1.00 (5.4e-3)
  f  both variants  0.96 - 0.96 (5.8e-3)  1.00 - 1.00 (3.8e-2)  1.00 - 1.00 (9.3e-3)  1.00 - 1.00 (6.7e-3)
(Row f was recorded over the five variants the test had then; three of them left with their kernels, the two that remain were among them.)
The ratio sits at 1.00 because the worst row is the same row in the kernel and in the emulation: its error is made by the bf16 roundings
themselves (a small gradient row left over from large rounded dS terms), which the two share; fp32 against float64 arithmetic moves it in
the third digit.  fp32 mode, worst row over all cases: O 2.9e-6, dq 3.9e-6, dk 8.0e-6, dv 3.3e-6 (bound 1e-4).  lse, worst token: 9.7e-7
(fp32), 9.9e-7 (bf16) (bound 1e-4).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_np as an  # noqa: E402
import _attention_worker as aw  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("O", "lse", "dq", "dk", "dv")


@functools.lru_cache(maxsize=None)
def _inputs(B, T, H, KV, hd, dtype, long_at="low", long_len=None):
    """operands of one case (bf16-exact when dtype == 1) and the tile classes of its rows"""
    rng = np.random.default_rng(B * 100003 + T * 101 + H * 7 + hd + dtype)
    qkv = rng.standard_normal((B * T, (H + 2 * KV) * hd)).astype(np.float32)
    dO = rng.standard_normal((B * T, H * hd)).astype(np.float32)
    if dtype == 1:
        qkv, dO = an.bf16_round(qkv), an.bf16_round(dO)
    uid, tm = an.make_users(B, T, B + T + hd, long_at, long_len)
    return {"qkv": qkv, "dO": dO, "uid": uid, "tm": tm, "classes": an.tile_classes(uid, tm)}


@functools.lru_cache(maxsize=None)
def _tables(rows, hd, identity=False):
    """cos / sin [rows][hd / 2]: theta uniform in [0, 2 pi) per (position, pair) -- no pair is near the identity; or the identity"""
    if identity:
        return np.ones((rows, hd // 2), np.float32), np.zeros((rows, hd // 2), np.float32)
    th = np.random.default_rng(rows * 131 + hd).uniform(0.0, 2 * np.pi, (rows, hd // 2))
    return np.cos(th).astype(np.float32), np.sin(th).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _positions(B, T, kind):
    rng = np.random.default_rng(B * 17 + T)
    if kind == "perm":        # a permutation of 0 .. T-1 per row
        return np.stack([rng.permutation(T) for _ in range(B)]).astype(np.int32)
    return rng.integers(0, 2 * T, (B, T)).astype(np.int32)      # "wide": anywhere in a table of 2 T rows


@functools.lru_cache(maxsize=None)
def _reference(key, H, KV, hd, rope, q_active):
    """(reference, bf16 emulation or None) of a case: computed once, shared by the tests on the same inputs, never modified.
    rope = (table rows, identity, position kind or None); q_active a tuple or None"""
    x = _inputs(*key)
    cos, sin = _tables(rope[0], hd, rope[1])
    pos = _positions(key[0], key[1], rope[2]) if rope[2] else None
    q, k, v = x["qkv"][:, :H * hd], x["qkv"][:, H * hd:(H + KV) * hd], x["qkv"][:, (H + KV) * hd:]
    args = (q, k, v, x["uid"], x["tm"], x["dO"], H, KV, hd, cos, sin, pos, q_active)
    ref = dict(zip(NAMES, an.attn_ref(*args)))
    emu = dict(zip(NAMES, an.attn_emul_bf16(*args))) if key[5] == 1 else None
    return ref, emu


def _launch(key, H, KV, hd, rope, q_active=None, dO=None, **kw):
    x = _inputs(*key)
    cos, sin = _tables(rope[0], hd, rope[1])
    pos = _positions(key[0], key[1], rope[2]) if rope[2] else None
    return aw.run_attention(key[5], H, KV, hd, x["qkv"], x["uid"], x["tm"], x["dO"] if dO is None else dO, cos, sin, pos,
                            None if q_active is None else np.array(q_active, np.int32), **kw)


def _compare(tag, res, ref, emu, key, H, KV, live=None):
    """every tensor of one launch against the reference: prints each figure, then asserts them all.  live (bool [B][T]): the tokens
    whose O / lse count (q_active); the gradients count everywhere."""
    B, T, bf = key[0], key[1], key[5] == 1
    flat = None if live is None else live.reshape(-1)
    bad = []
    for name, heads in (("O", H), ("dq", H), ("dk", KV), ("dv", KV)):
        rows = flat if name == "O" else None
        a, b = res[name], ref[name]
        e, (tok, head) = an.row_err(a, b, heads, rows)
        sel = slice(None) if rows is None else rows
        g = float(np.abs(np.nan_to_num(a[sel].astype(np.float64), nan=np.inf) - b[sel]).max() / np.abs(b[sel]).max()) if b[sel].size else 0.0
        E = an.row_err(emu[name], b, heads, rows)[0] if bf else 0.0
        bound, gbound = (2 * E, 3e-2) if bf else (1e-4, 2e-5)
        print(f"RATIO {tag} {'bf16' if bf else 'fp32'} {name}: e {e:.3e} at (b {tok // T}, token {tok % T}, head {head})  E {E:.3e}  "
              f"e/E {e / E if E else float('nan'):.2f}  whole-tensor {g:.3e}")
        if not (e <= bound and g <= gbound):
            bad.append((name, "row", e, "bound", bound, "at (b, token, head)", (tok // T, tok % T, head), "whole-tensor", g, "bound", gbound))
    e, where = an.lse_err(res["lse"], ref["lse"], live)
    lse_ref = ref["lse"] if live is None else ref["lse"][np.broadcast_to(live[:, None, :], ref["lse"].shape)]
    g = e / np.abs(lse_ref).max() if lse_ref.size else 0.0
    print(f"RATIO {tag} {'bf16' if bf else 'fp32'} lse: worst |a - b| {e:.3e} at (b, head, token) {where}  whole-tensor {g:.3e}")
    if not (e <= 1e-4 and g <= (3e-3 if bf else 1e-5)):
        bad.append(("lse", e, "bound 1e-4 at (b, head, token)", where, "whole-tensor", g))
    assert not bad, (tag, bad)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _need(c, *names):
    for n in names:
        assert c[n] >= 1, (n, c)


ALL4 = ("full", "partial", "empty", "idle_q16", "idle_k16")
SMALL = ("partial", "empty", "idle_q16", "idle_k16")       # T < 160: no room for a full pair (module docstring)


def ID(T):
    return (T, True, None)                                  # identity tables, implicit positions


# ---------------------------------------------------------------- a. tile classes
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("B,T,H,KV,hd", [(2, 328, 2, 1, 64), (8, 328, 8, 4, 64), (2, 328, 4, 2, 32), (2, 328, 2, 2, 16)])
def test_every_tile_class_against_the_reference(dtype, B, T, H, KV, hd):
    """Full, partial and empty tile pairs and idle 16-token groups in ONE launch: two heads per workgroup without the XCD lists (2 groups),
    with them (32 groups), and the register-staged kernels of head_dim 32 (paired heads) and 16 (one head per kv head); identity RoPE.
    bf16 / head_dim 64 runs attn_fwd_kernel<DMA>, attn_bwd_q_kernel<DMA> and attn_bwd_kv32_kernel, everything else the register-staged three."""
    key = (B, T, H, KV, hd, dtype)
    _need(_inputs(*key)["classes"], *ALL4)
    ref, emu = _reference(key, H, KV, hd, ID(T), None)
    _compare(f"a{key}", _launch(key, H, KV, hd, ID(T)), ref, emu, key, H, KV)


# ---------------------------------------------------------------- b. long rows: tile indices >= 16, bit 31
LONG = [(2040, "high", 64, 0), (2040, "high", 64, 1), (2048, "low", 64, 0), (2048, "low", 64, 1), (2040, "high", 32, 0)]


@pytest.mark.parametrize("T,long_at,hd,dtype", LONG)
def test_long_rows_use_the_high_tile_bits(T, long_at, hd, dtype):
    """32 tiles per row: every `1u << tile`, next_bit and the map words' bit 31.  T = 2040: the last tile has 56 tokens (the clamped
    min(token, T - 1) reads of its idle lanes) and the positions are an explicit permutation; T = 2048: implicit positions, the long
    user in the lower tiles and reaching past tile 16, so map words mix low and high bits.  Random-angle RoPE tables in both."""
    key = (1, T, 2, 1, hd, dtype, long_at)
    c = _inputs(*key)["classes"]
    _need(c, *ALL4, "full_hi", "partial_hi")
    assert 31 in c["q_tiles"] and 31 in c["k_tiles"], c
    rope = (T, False, "perm" if T == 2040 else None)
    ref, emu = _reference(key, 2, 1, hd, rope, None)
    _compare(f"b{key}", _launch(key, 2, 1, hd, rope), ref, emu, key, 2, 1)


@pytest.mark.parametrize("dtype", [0, 1])
def test_long_rows_compact_top_at_tile_31(dtype):
    """q_active = 31 of 32 tiles: `qa >= 32 ? all : (1 << qa) - 1` at its largest shift.  Tile 31's O and lse are NaN and its delta is
    NaN (the hook), its dO rows are zero: a dK/dV kernel that still visits query tile 31 turns the keys it sees NaN.  q_active = 32 must
    give the bits of the run without q_active."""
    T, H, KV, hd = 2048, 2, 1, 64
    key = (1, T, H, KV, hd, dtype, "low")
    c = _inputs(*key)["classes"]
    _need(c, *ALL4, "full_hi", "partial_hi")
    assert 31 in c["q_tiles"] and 31 in c["k_tiles"], c
    rope = (T, False, None)
    live = (np.arange(T)[None, :] // 64) < 31
    dO = _inputs(*key)["dO"] * live.reshape(-1, 1)
    res = _launch(key, H, KV, hd, rope, (31,), dO=dO, nan_out=True)
    ref, emu = _reference(key, H, KV, hd, rope, (31,))
    assert not res["raw_dqkv"][~live.reshape(-1), :H * hd].any()
    assert np.isfinite(res["dk"]).all() and np.isfinite(res["dv"]).all()
    _compare(f"b-top31{key}", res, ref, emu, key, H, KV, live)
    full, none = _launch(key, H, KV, hd, rope, (32,)), _launch(key, H, KV, hd, rope)
    for n in ("raw_O", "raw_dqkv", "lse"):
        assert _same_bits(full[n], none[n]), n


# ---------------------------------------------------------------- c. RoPE un-rotation
ROPE_SHAPES = [(2, 200, 2, 1, 64, 160), (1, 136, 2, 2, 32, None), (2, 328, 8, 4, 64, None)]
_identity_dv = {}


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("B,T,H,KV,hd,long_len,kind", [s + (k,) for s in ROPE_SHAPES for k in (None, "perm")] + [ROPE_SHAPES[0] + ("wide",)])
def test_rope_unrotation_of_dq_and_dk(dtype, B, T, H, KV, hd, long_len, kind):
    """dq and dk un-rotated with random-angle tables -- a sign or pairing slip at any un-rotation site (store_grad_tile for dQ and the
    register-staged dK, attn_bwd_kv32_kernel's own copy) moves every element -- with implicit positions, an explicit
    per-row permutation (the training step's top layer), and positions drawn from a table of 2 T rows.  dv is not rotated: it must equal
    the identity-table run's dv bit for bit."""
    key = (B, T, H, KV, hd, dtype, "low", long_len)
    _need(_inputs(*key)["classes"], *(ALL4 if T >= 160 else SMALL))
    rope = (2 * T if kind == "wide" else T, False, kind)
    ref, emu = _reference(key, H, KV, hd, rope, None)
    res = _launch(key, H, KV, hd, rope)
    _compare(f"c-{kind}{key}", res, ref, emu, key, H, KV)
    if key not in _identity_dv:
        _identity_dv[key] = _launch(key, H, KV, hd, ID(T))["raw_dqkv"][:, (H + KV) * hd:].copy()
    assert np.array_equal(res["raw_dqkv"][:, (H + KV) * hd:], _identity_dv[key])


# ---------------------------------------------------------------- d. the compact top (q_active)
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("B,T,H,KV,hd,qa", [(4, 328, 4, 2, 64, (0, 1, 3, 6)), (8, 328, 8, 4, 64, (6, 3, 1, 0, 1, 6, 3, 0))])
def test_compact_top_skips_inactive_query_tiles(dtype, B, T, H, KV, hd, qa):
    """q_active per row from {0, 1, 3, nt}: O / lse of the active tiles match; dq is exactly zero in the inactive tiles and matches
    elsewhere; dk / dv match the reference with the inactive dO rows zeroed and are finite although O, lse and delta of the inactive tiles
    are NaN (a kernel that reads one of them shows).  q_active = nt everywhere gives the bits of the run without it."""
    key = (B, T, H, KV, hd, dtype, "high")
    _need(_inputs(*key)["classes"], *ALL4)
    nt = (T + 63) // 64
    assert set(qa) == {0, 1, 3, nt}
    live = (np.arange(T)[None, :] // 64) < np.array(qa)[:, None]
    dO = _inputs(*key)["dO"] * live.reshape(-1, 1)
    res = _launch(key, H, KV, hd, ID(T), qa, dO=dO, nan_out=True)
    ref, emu = _reference(key, H, KV, hd, ID(T), qa)
    assert not res["raw_dqkv"][~live.reshape(-1), :H * hd].any()
    assert np.isfinite(res["dk"]).all() and np.isfinite(res["dv"]).all()
    _compare(f"d{key}", res, ref, emu, key, H, KV, live)
    full, none = _launch(key, H, KV, hd, ID(T), (nt,) * B), _launch(key, H, KV, hd, ID(T))
    for n in ("raw_O", "raw_dqkv", "lse"):
        assert _same_bits(full[n], none[n]), n


# ---------------------------------------------------------------- e. head shapes
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("B,T,H,KV,hd,long_len", [(1, 200, 2, 1, 128, 160), (2, 136, 4, 2, 128, None), (1, 136, 4, 1, 32, None), (1, 72, 8, 1, 16, None)])
def test_head_dim_128_and_wide_query_groups(dtype, B, T, H, KV, hd, long_len):
    """head_dim 128 forward AND backward (one head per workgroup even at two heads per kv head), and 4 / 8 query heads per kv head (the
    dK/dV kernels' item loop over the group's heads); random-angle RoPE, implicit positions."""
    key = (B, T, H, KV, hd, dtype, "low", long_len)
    _need(_inputs(*key)["classes"], *(ALL4 if T >= 160 else SMALL))
    rope = (T, False, None)
    ref, emu = _reference(key, H, KV, hd, rope, None)
    _compare(f"e{key}", _launch(key, H, KV, hd, rope), ref, emu, key, H, KV)


# ---------------------------------------------------------------- f. every kernel variant
VARIANTS = [("register-staged", {"RSYS_ATTN_DMA": "0"}),
            ("default", {})]


def test_every_kernel_variant_on_full_tiles_and_a_real_rotation(tmp_path):
    """bf16 / head_dim 64 behind the RSYS_ATTN_DMA switch (read once per process: one fresh child per variant, one at a time, each under
    its own time limit; the first abnormal exit ends the test).  Both variants against the reference on case (a)'s largest input with a
    permuted-position rotation; the register-staged and the LDS-DMA forward and dQ kernels run the same products in the same order, so
    O, lse and dQ must agree bit for bit -- now with the full-tile branches and the un-rotation in play (the default dK/dV kernel,
    attn_bwd_kv32_kernel, sums in another order and is held against the reference alone)."""
    B, T, H, KV, hd = 8, 328, 8, 4, 64
    key = (B, T, H, KV, hd, 1)
    x = _inputs(*key)
    _need(x["classes"], *ALL4)
    rope = (T, False, "perm")
    cos, sin = _tables(T, hd)
    src = str(tmp_path / "in.npz")
    np.savez(src, dtype=1, H=H, KV=KV, hd=hd, qkv=x["qkv"], dO=x["dO"], uid=x["uid"], tm=x["tm"], cos=cos, sin=sin, pos=_positions(B, T, "perm"))
    ref, emu = _reference(key, H, KV, hd, rope, None)
    base = {k: v for k, v in os.environ.items() if not k.startswith("RSYS_ATTN_")}
    outs = []
    for i, (name, env) in enumerate(VARIANTS):
        out = str(tmp_path / f"v{i}.npz")
        subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_attention_worker.py"), src, out, ROOT], check=True, env=dict(base, **env),
                       cwd=ROOT, timeout=120)
        outs.append(dict(np.load(out)))
    for (name, _), res in zip(VARIANTS, outs):
        _compare(f"f[{name}]", res, ref, emu, key, H, KV)
    for n in ("raw_O", "lse"):
        assert _same_bits(outs[0][n], outs[1][n]), n
    assert _same_bits(outs[0]["raw_dqkv"][:, :H * hd], outs[1]["raw_dqkv"][:, :H * hd]), "dq"


# ---------------------------------------------------------------- g. amax slots
@pytest.mark.parametrize("B,T,H,KV,hd", [(2, 328, 2, 1, 64), (8, 328, 8, 4, 64), (2, 328, 4, 2, 32), (2, 328, 2, 2, 16)])
def test_amax_slots_hold_the_largest_stored_magnitude(B, T, H, KV, hd):
    """the fp8 trunk's amax of O (forward) and dq / dk / dv (backward): the maximum over the 64 shards equals max |stored tensor| exactly"""
    key = (B, T, H, KV, hd, 1)
    _need(_inputs(*key)["classes"], *ALL4)
    res = _launch(key, H, KV, hd, ID(T), amax=True)
    want = np.array([np.abs(res[n]).max() for n in ("O", "dq", "dk", "dv")], np.float32)
    assert np.array_equal(res["amax"], want), (res["amax"], want)
