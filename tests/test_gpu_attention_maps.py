"""GPU: what launch_attn_tilemap (csrc/attention_maps.hip) writes -- the six tile maps, the two pair-bit matrices and the two launch orders --
read back through rsys_op_attention_maps and compared, entry by entry and with np.array_equal, with tests/_attention_np.py's tile_maps and
launch_orders.  The hook builds the maps the way rsys_op_attention_ex and rsys_op_attention_selected do before their first attention
kernel, and runs no attention kernel.  Everything is an integer: there is no tolerance.

The contract, both directions: a "some" bit is set if AND ONLY IF its tile (or 16-row group) has an allowed pair, a "full" bit if and only
if all 4096 pairs are allowed, qbits / kbits hold exactly the allowed matrix and its transpose, and each order list is THE stable
heaviest-first permutation of its slots' work under q_active (the identity where the launch takes its fallback).  The attention parity tests
hold only what changes O, lse or a gradient: a missed "some" bit, a false "full" bit, a wrong pair bit.

Every byte of the hook's map set holds 0xA5 before the first launch, so an entry the kernels leave unwritten shows; the order buffers are
compared over the lists and must still hold the fill behind them.  The dispatch facts (query heads per workgroup R, kv tile pairs, identity
fallback) stand as literals in the parameter lists and are checked against the hook's info; kv tile pairs needs the RSYS_ATTN_DMA switch on,
its default (the switch is read once per process: an ambient RSYS_ATTN_DMA=0 turns the expected value to 0)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_np as an  # noqa: E402

pytestmark = pytest.mark.gpu

FP32, BF16 = 0, 1
DMA_ON = os.environ.get("RSYS_ATTN_DMA", "") in ("", "1")   # (csrc/switches.hip: unset or empty = the default, on; the tests' own child sets 0)
ERR_ARG = -1
FILL32 = np.uint32(0xA5A5A5A5)
MAPS = ("qmap", "kmap", "qmap_full", "kmap_full", "qmap16", "kmap16", "qbits", "kbits")
PATTERNS = ("users_low", "users_high", "one_user", "own", "edges", "interleaved", "extreme", "pad_row")


@functools.lru_cache(maxsize=None)
def _tokens(name, B, T):
    """uid, tm [B][T] int32 of a named token pattern (read-only: shared between tests)"""
    t = np.arange(T)
    if name in ("users_low", "users_high"):
        uid, tm = an.make_users(B, T, 7 + T, name[6:])
    elif name == "one_user":          # everything allowed: every tile full except the ragged one
        uid, tm = np.full((B, T), 77, np.int32), np.zeros((B, T), np.int32)
    elif name == "own":               # every token its own user: only the diagonal
        uid = np.broadcast_to(t[None, :] + 1, (B, T)).astype(np.int32); tm = np.full((B, T), 3, np.int32)
    elif name == "edges":             # users that end at a multiple of 16 (so also of 64), one token before it or one behind it, by row
        uid = np.zeros((B, T), np.int32); tm = np.zeros((B, T), np.int32)
        for b in range(B):
            cuts = [m + (m // 16 + b) % 3 - 1 for m in range(16, T, 16)]
            uid[b] = np.searchsorted(np.array(cuts, np.int64), t, side="right") + 1 + 100 * b
            if cuts:
                tm[b, np.array(cuts) % T] = 1 + (np.arange(len(cuts)) % 3)
    elif name == "interleaved":       # masked and unmasked tokens alternate inside two users: allowed(q, k) != allowed(k, q)
        uid = np.where(t[None, :] < (2 * T) // 3, 5, 6).astype(np.int32) + np.zeros((B, 1), np.int32)
        tm = np.where(t % 2 == 1, 9 + (t // 2) % 2, 0).astype(np.int32)[None, :] + np.zeros((B, 1), np.int32)
    elif name == "extreme":           # the largest and the smallest token key
        run = (t // 24 + np.arange(B)[:, None]) % 2 == 0
        uid = np.where(run, 2 ** 19 - 1, 0).astype(np.int32)
        tm = np.where(run & (t % 3 != 0)[None, :], 4095, 0).astype(np.int32)
    elif name == "pad_row":           # row 0 entirely the pad user
        uid, tm = an.make_users(B, T, 3 + T, "high")
        uid[0] = 0; tm[0] = 0
    else:
        raise KeyError(name)
    uid = np.ascontiguousarray(uid, np.int32); tm = np.ascontiguousarray(tm, np.int32)
    assert uid.shape == tm.shape == (B, T) and uid.min() >= 0 and uid.max() < 2 ** 19 and tm.min() >= 0 and tm.max() < 4096
    uid.setflags(write=False); tm.setflags(write=False)
    return uid, tm


@functools.lru_cache(maxsize=None)
def _expected(name, B, T):
    """tile_maps of a named pattern: computed once, shared, never modified"""
    m = an.tile_maps(*_tokens(name, B, T))
    for a in m.values():
        a.setflags(write=False)
    return m


def _call(dtype, B, T, H, KV, hd, uid, tm, q_active=None, prev=None):
    """one rsys_op_attention_maps call -> (rc, outputs by name); the host outputs start as 0x5C bytes"""
    from recommendersystem_amd import _lib
    lib = _lib.lib()
    ptrs = []

    def dev(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.int32)
        p = C.c_void_p()
        assert lib.rsys_dev_alloc(C.byref(p), max(a.nbytes, 4)) == 0
        assert lib.rsys_dev_h2d(p, a.ctypes.data, a.nbytes) == 0
        ptrs.append(p)
        return p

    nt = (max(T, 1) + 63) // 64
    W = np.uint32 if nt <= 32 else np.uint64
    out = {k: np.empty((B, nt), W) for k in MAPS[:4]}
    out["qmap16"] = np.empty((B, nt, 4), W); out["kmap16"] = np.empty((B, nt, 4), W)
    out["qbits"] = np.empty((B, nt, nt, 64), np.uint64); out["kbits"] = np.empty((B, nt, nt, 64), np.uint64)
    out["order_q"] = np.empty(B * H * nt, np.int32); out["order_k"] = np.empty(B * KV * nt, np.int32)
    out["info"] = np.empty(8, np.int32)
    for a in out.values():
        a.view(np.uint8)[...] = 0x5C
    args = [dev(np.reshape(uid, -1)), dev(np.reshape(tm, -1)), dev(q_active)]
    args += [dev(np.reshape(prev[0], -1)), dev(np.reshape(prev[1], -1))] if prev is not None else [None, None]
    args += [out[k].ctypes.data for k in MAPS + ("order_q", "order_k", "info")]
    rc = lib.rsys_op_attention_maps(dtype, B, T, H, KV, hd, *args)
    for p in ptrs:
        lib.rsys_dev_free(p)
    return rc, out


def _check(tag, dtype, B, T, H, KV, hd, uid, tm, want, R, kv_pairs, identity, q_active=None, prev=None):
    """the hook's ten arrays and its info against the restatement (`want` = tile_maps(uid, tm)); returns the expected orders and their keys"""
    from recommendersystem_amd import _lib
    rc, got = _call(dtype, B, T, H, KV, hd, uid, tm, q_active, prev)
    assert rc == 0, _lib.last_error()
    nt = (T + 63) // 64
    kv_pairs = int(bool(kv_pairs) and DMA_ON)
    lists = 8 if B * KV % 8 == 0 else 1
    n_inner_q, n_inner_k = (H // KV // R) * nt, (nt + 1) // 2 if kv_pairs else nt
    assert got["info"].tolist() == [1 if nt <= 32 else 2, R, kv_pairs, int(lists == 8), n_inner_q, n_inner_k, int(identity), nt], (tag, got["info"])
    for k in MAPS:
        if not np.array_equal(got[k], want[k]):
            bad = np.argwhere(got[k] != want[k])
            i = tuple(bad[0])
            raise AssertionError(f"{tag}: {k} differs in {len(bad)} entries; first at {i}: device {int(got[k][i]):#x}, expected {int(want[k][i]):#x}")
    keys = an.order_keys(want["qmap"], want["kmap"], B, T, H, KV, R, kv_pairs, q_active)
    orders = an.launch_orders(want["qmap"], want["kmap"], B, T, H, KV, R, kv_pairs, q_active, identity=bool(identity))
    for k, o, n_inner in (("order_q", orders[0], n_inner_q), ("order_k", orders[1], n_inner_k)):
        assert o.shape == (lists, B * KV // lists * n_inner)
        n = o.size
        if not np.array_equal(got[k][:n], o.reshape(-1)):
            bad = np.nonzero(got[k][:n] != o.reshape(-1))[0]
            raise AssertionError(f"{tag}: {k} differs in {len(bad)} of {n} slots; first at {int(bad[0])}: device {int(got[k][bad[0]])}, expected "
                                 f"{int(o.reshape(-1)[bad[0]])}")
        assert (got[k][n:].view(np.uint32) == FILL32).all(), (tag, k, "written behind its lists")
    return orders, keys


def _q_active(kind, B, nt):
    if kind is None:
        return None
    if kind == "zero":
        return np.zeros(B, np.int32)
    if kind == "all":
        return np.full(B, nt, np.int32)
    assert kind == "mix"
    return np.array(([1, nt, max(nt // 2, 1), 0, nt - 1 if nt > 1 else 1] * B)[:B], np.int32)


# ---------------------------------------------------------------- the map words at every row length
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("T", [8, 64, 72])
def test_one_and_two_tiles(T, pattern):
    """one ragged tile, one exact tile, two tiles with a ragged last"""
    B, H, KV, hd = 3, 2, 1, 64
    uid, tm = _tokens(pattern, B, T)
    _check(f"{pattern} T{T}", BF16, B, T, H, KV, hd, uid, tm, _expected(pattern, B, T), 2, 1, 0, _q_active("mix", B, (T + 63) // 64))


@pytest.mark.parametrize("q_active", [None, "zero", "all", "mix"])
@pytest.mark.parametrize("B,H,KV", [(2, 8, 4), (3, 4, 1)])
@pytest.mark.parametrize("long_at", ["low", "high"])
def test_every_tile_class_at_the_parity_size(long_at, B, H, KV, q_active):
    """make_users at T = 328 (the parity tests' rows): every class, eight XCD lists and one list, every kind of q_active"""
    T, hd, nt = 328, 64, 6
    name = "users_" + long_at
    uid, tm = _tokens(name, B, T)
    c = an.tile_classes(uid, tm)
    assert min(c["full"], c["partial"], c["empty"], c["idle_q16"], c["idle_k16"]) >= 1, c
    want = _expected(name, B, T)
    qa = _q_active(q_active, B, nt)
    R = 2 if H // KV == 2 else 1
    orders, keys = _check(f"{name} B{B} {q_active}", BF16, B, T, H, KV, hd, uid, tm, want, R, 1, 0, qa)
    if q_active == "mix" and long_at == "high":
        # row 0 has one active query tile: a kv tile that only inactive query tiles see has no work on the k side
        assert qa[0] == 1 and ((want["kmap"][0] != 0) & (want["kmap"][0] & np.uint32(1) == 0)).any()
    if q_active == "zero":
        assert not keys[0].any() and not keys[1].any() and (orders[0] == np.arange(orders[0].shape[1])).all()
    if q_active in (None, "all") and long_at == "high":
        assert any((o != np.arange(o.shape[1])).any() for o in orders), "the sorted order is the identity: this case holds nothing"


@pytest.mark.parametrize("pattern,q_active", [("users_low", None), ("users_high", "mix"), ("edges", None), ("interleaved", "mix")])
@pytest.mark.parametrize("B,H,KV,R", [(2, 8, 4, 2), (3, 2, 1, 2)])
@pytest.mark.parametrize("T", [2048, 2056, 4088, 4096])
def test_word_width_edges(T, B, H, KV, R, pattern, q_active):
    """bit 31 of the 32-bit words, the first row length with 64-bit words (33 tiles), 64 tiles with a ragged last one, bit 63; the XCD-list
    form (B * KV = 8) and the single list with wide words"""
    nt = (T + 63) // 64
    uid, tm = _tokens(pattern, B, T)
    want = _expected(pattern, B, T)
    assert want["qmap"].dtype == (np.uint32 if nt <= 32 else np.uint64)
    assert ((want["qmap"][:, nt - 1] >> want["qmap"].dtype.type(nt - 1)) & 1).all()      # the word's highest bit in use
    if pattern == "users_low":
        assert want["qmap_full"].any() and (want["qmap"] & ~want["qmap_full"]).any()
    _check(f"{pattern} T{T} B{B}", BF16, B, T, H, KV, 64, uid, tm, want, R, 1, 0, _q_active(q_active, B, nt))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("T", [328, 2056])
def test_token_patterns(T, pattern):
    B, H, KV, hd = 3, 4, 2, 32
    uid, tm = _tokens(pattern, B, T)
    want = _expected(pattern, B, T)
    nt = (T + 63) // 64
    if pattern == "one_user":
        full = an.popcount(want["qmap_full"])
        assert (full[:, :nt - 1] == nt - 1).all() and (full[:, nt - 1] == 0).all()      # T is ragged: everything full except the last tile
    if pattern == "own":
        assert (an.popcount(want["qmap"]) == 1).all() and (an.popcount(want["qbits"]).sum((2, 3)) == np.minimum(64, T - 64 * np.arange(nt))).all()
    if pattern == "interleaved":
        a = an.allowed_pairs(uid[:, :64], tm[:, :64])
        assert (a != a.transpose(0, 2, 1)).any()
    if pattern == "pad_row":
        assert not uid[0].any() and not tm[0].any()
    _check(f"{pattern} T{T}", FP32, B, T, H, KV, hd, uid, tm, want, 2, 0, 0)


# ---------------------------------------------------------------- dispatch facts
@pytest.mark.parametrize("H,KV,hd,dtype,R,kv_pairs", [(2, 1, 64, BF16, 2, 1), (8, 4, 64, FP32, 2, 0), (4, 2, 128, BF16, 1, 0), (4, 1, 32, BF16, 1, 0),
                                                      (2, 2, 16, BF16, 1, 0)])
def test_heads_per_workgroup(H, KV, hd, dtype, R, kv_pairs):
    """R = 2 only for H / KV = 2 with hd <= 64"""
    B, T = 2, 328
    uid, tm = _tokens("users_high", B, T)
    _check(f"H{H} KV{KV} hd{hd}", dtype, B, T, H, KV, hd, uid, tm, _expected("users_high", B, T), R, kv_pairs, 0, _q_active("mix", B, 6))


@pytest.mark.parametrize("dtype,hd,kv_pairs", [(BF16, 64, 1), (FP32, 64, 0), (BF16, 32, 0), (BF16, 128, 0)])
@pytest.mark.parametrize("B,H,KV", [(2, 8, 4), (3, 2, 1)])
@pytest.mark.parametrize("T", [8, 72, 136, 328, 2056])
def test_kv_tile_pairs(T, B, H, KV, dtype, hd, kv_pairs):
    """order_k lists PAIRS of kv tiles only for bf16 at hd = 64; nt = 1, 3 and 33 leave the last pair without its second tile"""
    nt = (T + 63) // 64
    uid, tm = _tokens("users_high", B, T)
    R = 2 if hd <= 64 else 1
    _check(f"T{T} B{B} hd{hd}", dtype, B, T, H, KV, hd, uid, tm, _expected("users_high", B, T), R, kv_pairs, 0, _q_active("mix", B, nt))


def test_kv_tile_pairs_follow_the_dma_switch():
    """RSYS_ATTN_DMA=0 -- read once per process, so a fresh child (this file as a program) --: bf16 at hd = 64 lists single kv tiles"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, RSYS_ATTN_DMA="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "MAPS_CHILD_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------- ties, reuse, the identity fallback
@pytest.mark.parametrize("B,H,KV,R", [(4, 4, 2, 2), (3, 4, 1, 1)])
@pytest.mark.parametrize("T", [328, 2056])
def test_identical_rows_keep_slot_order(T, B, H, KV, R):
    """every row the same: per tile index all keys are equal, so that stability decides the whole order"""
    u1, t1 = _tokens("users_high", 1, T)
    uid = np.repeat(u1, B, 0); tm = np.repeat(t1, B, 0)
    w1 = _expected("users_high", 1, T)
    want = {k: np.repeat(v, B, 0) for k, v in w1.items()}
    orders, keys = _check(f"ties T{T} B{B}", BF16, B, T, H, KV, 64, uid, tm, want, R, 1, 0)
    for k in keys:
        assert max(np.unique(row, return_counts=True)[1].max() for row in k) >= B * KV // (8 if B * KV % 8 == 0 else 1)


@pytest.mark.parametrize("first,second", [("one_user", "own"), ("own", "one_user"), ("users_low", "users_high")])
@pytest.mark.parametrize("T", [328, 2056])
def test_a_reused_map_set_keeps_nothing_of_the_step_before(T, first, second):
    """launch on `first`, then on `second` into the same map set, as a model does step after step: the maps are those of `second` alone"""
    B, H, KV, hd = 2, 8, 4, 64
    uid, tm = _tokens(second, B, T)
    w1, w2 = _expected(first, B, T), _expected(second, B, T)
    assert any((w1[k] & ~w2[k]).any() for k in ("kmap", "kmap_full", "qmap_full", "kmap16")) or first == "own"   # bits that must go
    _check(f"{first} then {second} T{T}", BF16, B, T, H, KV, hd, uid, tm, w2, 2, 1, 0, None, _tokens(first, B, T))


@functools.lru_cache(maxsize=None)
def _varied(B, T):
    """sparse rows with different work per tile: users of 16 tokens with shifted edges, the first row one user in its first 256 tokens"""
    uid, tm = _tokens("edges", B, T)
    uid = uid.copy(); tm = tm.copy()
    uid[0, :256] = 9000
    uid[1::3, 100:400] = 9001
    return uid, tm


@pytest.mark.parametrize("B,T,H,slots,chunks,identity", [(5, 4096, 40, 12800, 200, 0), (3, 4096, 67, 12864, 201, 1), (13, 2112, 32, 13728, 215, 1),
                                                         (20, 2048, 40, 25600, 400, 0), (9, 2048, 89, 25632, 401, 1)])
def test_identity_fallback_at_the_chunk_cap(B, T, H, slots, chunks, identity):
    """one list of B * H * nt slots (KV = 1) in chunks of 64: 200 chunks of wide words and 400 of 32-bit words are sorted, one chunk more
    falls back to the identity"""
    nt = (T + 63) // 64
    assert B * H * nt == slots and (slots + 63) // 64 == chunks and (chunks > (200 if nt > 32 else 400)) == bool(identity)
    uid, tm = _varied(B, T)
    want = an.tile_maps(uid, tm)
    qa = _q_active("mix", B, nt)
    orders, keys = _check(f"cap B{B} T{T} H{H}", FP32, B, T, H, 1, 16, uid, tm, want, 1, 0, identity, qa)
    srt = an.launch_orders(want["qmap"], want["kmap"], B, T, H, 1, 1, 0, qa)
    for o in srt:                                             # (sorted and identity differ here, on either side)
        assert (o != np.arange(o.shape[1])).any()


# ---------------------------------------------------------------- argument errors
@pytest.mark.parametrize("what", ["uid_high", "tm_high", "uid_negative", "tm_negative", "T_not_8", "T_long", "q_active_negative", "q_active_high",
                                  "prev_uid_high", "prev_tm_negative"])
def test_argument_errors_launch_nothing(what):
    B, T, H, KV, hd = 2, 72, 2, 1, 64
    if what == "T_not_8":
        T = 68
    if what == "T_long":
        T = 4104
    uid = np.ones((B, T), np.int32); tm = np.zeros((B, T), np.int32)
    prev = [uid.copy(), tm.copy()] if what.startswith("prev") else None
    qa = None
    if what == "uid_high":
        uid[1, T - 1] = 2 ** 19
    if what == "tm_high":
        tm[1, 3] = 4096
    if what == "uid_negative":
        uid[0, 0] = -1
    if what == "tm_negative":
        tm[1, T - 1] = -1
    if what == "prev_uid_high":
        prev[0][0, 5] = 2 ** 19
    if what == "prev_tm_negative":
        prev[1][1, 5] = -4096
    if what == "q_active_negative":
        qa = np.array([1, -1], np.int32)
    if what == "q_active_high":
        qa = np.array([3, 2], np.int32)
    rc, got = _call(BF16, B, T, H, KV, hd, uid, tm, qa, prev)
    assert rc == ERR_ARG, (what, rc)
    for k, a in got.items():
        assert (a.view(np.uint8) == 0x5C).all(), (what, k, "written")
    if not what.startswith("T_"):                            # the same call without the violation is fine
        ok = np.ones((B, T), np.int32)
        rc, got = _call(BF16, B, T, H, KV, hd, ok, np.zeros((B, T), np.int32), np.array([2, 0], np.int32) if qa is not None else None)
        assert rc == 0 and got["info"][7] == 2


if __name__ == "__main__":   # the child of test_kv_tile_pairs_follow_the_dma_switch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert not DMA_ON, "run with RSYS_ATTN_DMA=0"
    for T_ in (136, 328):
        u_, t_ = _tokens("users_high", 2, T_)
        _check(f"switch off T{T_}", BF16, 2, T_, 8, 4, 64, u_, t_, _expected("users_high", 2, T_), 2, 0, 0, _q_active("mix", 2, (T_ + 63) // 64))
    print("MAPS_CHILD_OK")
