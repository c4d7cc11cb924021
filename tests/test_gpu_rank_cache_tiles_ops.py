"""GPU: the two kernels of the packed ranking cache alone, through their hooks (rsys_debug.h).  attn_cand_tiles_kernel
(rsys_op_attention_cached_tiles): every live tile bit-equal to attn_cand_kernel (rsys_op_attention_cached) on a row that holds the segment
at its start, fp32 against a float64 soft-max, dead tiles and the zeroed tail, and cache rows nobody may read filled with NaN.
rank_cache_copy_segments_kernel (rsys_op_rank_cache_copy_segments): the slots' contents bit for bit and a sentinel everywhere else."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ROWS, T, NT = 2, 256, 4            # two rows of four 64-token tiles
N_SLOTS = 8
# (row, first_tile, n_cand, slot, n_hist): n_hist 0 / 1 / 31 / 32 / 33 / 63, n_cand 1 / 31 / 32 / 33 / 64 (two tiles), slot 3 read twice;
# tile 1 of row 0 and tile 2 of row 1 are dead; slots 6 and 7 are used by nobody
SEGMENTS = [(0, 0, 1, 0, 0), (0, 2, 64, 1, 31), (1, 0, 31, 2, 1), (1, 1, 32, 3, 63), (1, 3, 32, 3, 63)]
# a second launch covers the remaining counts: n_cand 33 (a tile and one pair), n_hist 32 and 33; tiles 2 and 3 of row 0, tile 3 of row 1 dead
SEGMENTS_B = [(0, 0, 33, 4, 32), (1, 0, 1, 5, 33), (1, 1, 31, 4, 32), (1, 2, 1, 5, 33)]
CASES = [(hd, rep, kv, dt) for hd in (16, 32, 64, 128) for rep in (1, 2) for kv in (1,) for dt in (0, 1)] + [(64, 2, 2, 0), (64, 2, 2, 1), (32, 1, 3, 1)]


def _bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def _pack(a, bf):
    a = np.ascontiguousarray(a, np.float32)
    return (a.view(np.uint32) >> 16).astype(np.uint16) if bf else a


def _unpack(raw, bf):
    return (raw.astype(np.uint32) << 16).view(np.float32) if bf else raw


class Dev:
    """device buffers of one test, freed together"""
    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.lib.rsys_dev_alloc(C.byref(p), max(a.nbytes, 16)) == 0
        assert self.lib.rsys_dev_h2d(p, a.ctypes.data, a.nbytes) == 0
        self.ptrs.append(p)
        return p

    def get(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        assert self.lib.rsys_dev_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def free(self):
        for p in self.ptrs:
            self.lib.rsys_dev_free(p)


def _ref64(qkv, cache, seg, H, KV, hd):
    """float64 soft-max per segment: candidate j's two tokens see the slot's 2 n_hist cached tokens and themselves"""
    rep = H // KV
    x = qkv.reshape(ROWS, T, -1).astype(np.float64)
    out = {}
    for i, (r, ft, nc, sl, nh) in enumerate(seg):
        ck = cache[sl, :2 * nh, :KV * hd].reshape(-1, KV, hd).astype(np.float64)
        cv = cache[sl, :2 * nh, KV * hd:].reshape(-1, KV, hd).astype(np.float64)
        o = np.zeros((2 * nc, H, hd))
        for j in range(nc):
            tok = slice(64 * ft + 2 * j, 64 * ft + 2 * j + 2)
            q = x[r, tok, :H * hd].reshape(2, H, hd)
            keys = np.concatenate([ck, x[r, tok, H * hd:(H + KV) * hd].reshape(2, KV, hd)], 0)
            vals = np.concatenate([cv, x[r, tok, (H + KV) * hd:].reshape(2, KV, hd)], 0)
            for h in range(H):
                s = q[:, h] @ keys[:, h // rep].T / np.sqrt(hd)
                p = np.exp(s - s.max(-1, keepdims=True)); p /= p.sum(-1, keepdims=True)
                o[2 * j:2 * j + 2, h] = p @ vals[:, h // rep]
        out[i] = o.reshape(2 * nc, H * hd)
    return out


@pytest.mark.parametrize("seg", [SEGMENTS, SEGMENTS_B], ids=["a", "b"])
@pytest.mark.parametrize("hd,rep,KV,dtype", CASES)
def test_tiles_kernel_against_the_row_kernel(hd, rep, KV, dtype, seg):
    from recommendersystem_amd import _lib
    lib = _lib.lib()
    dev = Dev(lib)
    bf = dtype == 1
    H = KV * rep
    Nq, kvw, No = (H + 2 * KV) * hd, 2 * KV * hd, H * hd
    rng = np.random.default_rng(7000 + 100 * hd + 10 * rep + 2 * KV + dtype)
    qkv = rng.standard_normal((ROWS * T, Nq)).astype(np.float32)
    cache = rng.standard_normal((N_SLOTS, T, kvw)).astype(np.float32)
    if bf:
        qkv, cache = _bf16_round(qkv), _bf16_round(cache)
    raw_t = np.uint16 if bf else np.float32
    sentinel = np.full((ROWS * T, No), 7.0, np.float32)
    d_qkv, d_cache = dev.put(_pack(qkv, bf)), dev.put(_pack(cache, bf))
    d_O = dev.put(_pack(sentinel, bf))
    segs = np.array(seg, np.int32)
    rc = lib.rsys_op_attention_cached_tiles(dtype, ROWS, T, H, KV, hd, d_qkv, d_cache, N_SLOTS, 0, len(seg), segs.ctypes.data, d_O)
    assert rc == 0, _lib.last_error()
    raw = dev.get(d_O, (ROWS, T, No), raw_t)
    O = _unpack(raw, bf)

    # (a) bit-equal to the row kernel on rows that hold each segment at their start (one row per segment, one launch)
    n = len(seg)
    rows_qkv = np.zeros((n, T, Nq), np.float32)
    for i, (r, ft, nc, sl, nh) in enumerate(seg):
        tiles = -(-2 * nc // 64)
        rows_qkv[i, :64 * tiles] = qkv.reshape(ROWS, T, Nq)[r, 64 * ft:64 * (ft + tiles)]
    d_rq = dev.put(_pack(rows_qkv.reshape(n * T, Nq), bf)); d_rO = dev.put(_pack(np.full((n * T, No), 7.0, np.float32), bf))
    d_sl, d_nh, d_nc = dev.put(segs[:, 3].copy()), dev.put(segs[:, 4].copy()), dev.put(segs[:, 2].copy())
    rc = lib.rsys_op_attention_cached(dtype, n, T, H, KV, hd, d_rq, d_cache, N_SLOTS, d_sl, d_nh, d_nc, d_rO)
    assert rc == 0, _lib.last_error()
    row_raw = dev.get(d_rO, (n, T, No), raw_t)
    live_tile = np.zeros((ROWS, NT), bool)
    for i, (r, ft, nc, sl, nh) in enumerate(seg):
        tiles = -(-2 * nc // 64)
        live_tile[r, ft:ft + tiles] = True
        assert np.array_equal(raw[r, 64 * ft:64 * (ft + tiles)], row_raw[i, :64 * tiles]), f"segment {i}: not the row kernel's bits"
        # (c) rows >= 2 n_cand of the segment's last tile: exact zeros
        assert np.all(raw[r, 64 * ft + 2 * nc:64 * (ft + tiles)] == 0)
    assert not live_tile.all(axis=1).any(), "every row keeps a dead tile"
    # (c) dead tiles keep the sentinel
    sent_raw = _pack(sentinel, bf).reshape(ROWS, NT, 64, No)
    assert np.array_equal(raw.reshape(ROWS, NT, 64, No)[~live_tile], sent_raw[~live_tile])

    # (b) fp32: against a float64 soft-max
    if not bf:
        ref = _ref64(qkv, cache, seg, H, KV, hd)
        err = max(float(np.abs(O[r, 64 * ft:64 * ft + 2 * nc] - ref[i]).max() / np.abs(ref[i]).max()) for i, (r, ft, nc, _, _) in enumerate(seg))
        print(f"attn_cand_tiles fp32 hd {hd} H/KV {rep} KV {KV}: err {err:.3e}")
        assert err < 1e-4, err

    # (d) cache rows past every slot's 2 n_hist and every unused slot: NaN.  The output is finite and unchanged.
    poisoned = np.full_like(cache, np.nan)
    for _, _, _, sl, nh in seg:
        poisoned[sl, :2 * nh] = cache[sl, :2 * nh]
    d_pc = dev.put(_pack(poisoned, bf)); d_O2 = dev.put(_pack(sentinel, bf))
    rc = lib.rsys_op_attention_cached_tiles(dtype, ROWS, T, H, KV, hd, d_qkv, d_pc, N_SLOTS, 0, len(seg), segs.ctypes.data, d_O2)
    assert rc == 0, _lib.last_error()
    raw2 = dev.get(d_O2, (ROWS, T, No), raw_t)
    assert np.isfinite(_unpack(raw2, bf)).all() and np.array_equal(raw, raw2)
    dev.free()


def test_tiles_hook_refuses_bad_segments():
    from recommendersystem_amd import _lib
    lib = _lib.lib()
    dev = Dev(lib)
    H = KV = 1; hd = 16
    d_qkv = dev.put(np.zeros((ROWS * T, 3 * hd), np.float32)); d_cache = dev.put(np.zeros((N_SLOTS, T, 2 * hd), np.float32))
    sentinel = np.full((ROWS * T, hd), 7.0, np.float32)
    d_O = dev.put(sentinel)
    for bad in ([(2, 0, 1, 0, 0)], [(0, 4, 1, 0, 0)], [(0, 3, 33, 0, 0)], [(0, 0, 0, 0, 0)], [(0, 0, 1, N_SLOTS, 0)], [(0, 0, 1, 0, T // 2 + 1)],
                [(0, 0, 33, 0, 0), (0, 1, 1, 1, 0)]):
        segs = np.array(bad, np.int32)
        assert lib.rsys_op_attention_cached_tiles(0, ROWS, T, H, KV, hd, d_qkv, d_cache, N_SLOTS, 0, len(bad), segs.ctypes.data, d_O) == -1, bad
    assert np.array_equal(dev.get(d_O, sentinel.shape, np.float32), sentinel)
    dev.free()


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("H,KV,hd", [(1, 1, 16), (2, 1, 64), (4, 2, 32), (2, 2, 128)])
def test_copy_segments_kernel(H, KV, hd, dtype):
    """(row, first column, n_hist, slot): histories of 0 / 1 / 31 / 32 / 33 / 63 events at columns 0 / 32 / 64 / 96 of two rows into slots of
    Tc = 320 tokens (longer than a row, as a trimmed batch's); the slot rows [0, 2 n_hist) are the source tokens' K | V bit for bit, every
    other value of the cache keeps its sentinel"""
    from recommendersystem_amd import _lib
    lib = _lib.lib()
    dev = Dev(lib)
    bf = dtype == 1
    Tc = 320
    seg = [(0, 0, 31, 5), (0, 32, 0, 1), (0, 64, 63, 0), (1, 0, 1, 7), (1, 32, 32, 2), (1, 64, 33, 4)]
    Nq, kvw = (H + 2 * KV) * hd, 2 * KV * hd
    rng = np.random.default_rng(300 + hd + dtype)
    raw_t = np.uint16 if bf else np.float32
    qkv = _pack(rng.standard_normal((ROWS, T, Nq)).astype(np.float32), bf)
    cache0 = _pack(np.full((N_SLOTS, Tc, kvw), 7.0, np.float32), bf)
    d_qkv, d_cache = dev.put(qkv), dev.put(cache0)
    segs = np.array(seg, np.int32)
    rc = lib.rsys_op_rank_cache_copy_segments(dtype, ROWS, T, H, KV, hd, d_qkv, d_cache, N_SLOTS, Tc, len(seg), segs.ctypes.data)
    assert rc == 0, _lib.last_error()
    got = dev.get(d_cache, cache0.shape, raw_t)
    want = cache0.copy()
    for r, c0, nh, sl in seg:
        want[sl, :2 * nh] = qkv[r, 2 * c0:2 * c0 + 2 * nh, H * hd:]
    assert np.array_equal(got, want)
    # refused before any launch: a segment across the row's end, a slot outside the cache, a history longer than a slot
    for bad in ((0, 96, 33, 0), (0, 0, 1, N_SLOTS), (2, 0, 1, 0), (0, -32, 1, 0)):
        b = np.array([bad], np.int32)
        assert lib.rsys_op_rank_cache_copy_segments(dtype, ROWS, T, H, KV, hd, d_qkv, d_cache, N_SLOTS, Tc, 1, b.ctypes.data) == -1, bad
    assert np.array_equal(dev.get(d_cache, cache0.shape, raw_t), want)
    dev.free()
