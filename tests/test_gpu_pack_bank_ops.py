"""GPU: the adapter bank's two forward kernels with a slot per 64-token tile (csrc/adapter_bank.hip: adapter_bank_a_kernel /
adapter_bank_b_kernel with a tile map in their BankLookup) through rsys_op_adapter_bank_tiles, bit for bit against the same
kernels with a slot per row: the two lookup paths of one kernel pinned against each other.

The expected output needs no arithmetic of its own: for every slot s the tile map names, rsys_op_adapter_bank runs with row_slot = s on
every row, and each 64-token tile is taken from the run of its slot.  La and the q and v columns of qkv must be equal bit for bit; tiles
with -1, the k columns and the sentinel tails behind every buffer must be unwritten.

  Ttok  D   H KV hd   tiles   what it reaches
     8   16  1 1  16    1     a lone partial tile (half a stage-A work item)
    72  160  5 1  32    2     a tile boundary with Ttok % 16 == 8: the second tile holds 8 tokens, one stage-B item and half a stage-A item
   136  320  5 5  64    3     three tiles, the last of 8 tokens; stage B loops (8 tokens x 80 items > 256 threads)
   128  128  2 1  64    2     the regular shape of the whole-model tests

rows = 3.  Tile maps: different slots in neighbouring tiles, a -1 tile between two live ones (three tiles), a row of all -1, slot 7."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_adapter_bank_ops import Bufs, rope_tables, same
from test_gpu_row_kernels import BF16, F32, SENT, _lib, storage

pytestmark = pytest.mark.gpu

ROWS, LAYERS, LAYER, SLOTS = 3, 2, 1, 8
CASES = {1: (8, 16, 1, 1, 16), 2: (72, 160, 5, 1, 32), 3: (136, 320, 5, 5, 64), 4: (128, 128, 2, 1, 64)}
TILES = {1: [[3], [-1], [7]], 2: [[3, 7], [-1, -1], [0, -1]], 3: [[3, -1, 7], [-1, -1, -1], [0, 3, 5]]}
A, B = 1, 2


def dims(case):
    T, D, H, KV, hd = CASES[case]
    return T, D, H, KV, hd, H * hd, KV * hd, (H + 2 * KV) * hd


def tile_map(case):
    return np.asarray(TILES[-(-CASES[case][0] // 64)], np.int32)


@functools.lru_cache(maxsize=None)
def problem(case, dt):
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    rng = np.random.default_rng(900 + 10 * case + dt)
    c = {"xn": storage(rng.standard_normal((ROWS, T, D)), dt), "qkv": storage(rng.standard_normal((ROWS, T, ld)), dt),
         "La_in": storage(rng.standard_normal((ROWS, T, 16)), dt),          # stage B alone reads a given La
         "bankA": storage(0.1 * rng.standard_normal((SLOTS, LAYERS, 16, D)), dt),
         "bankB": storage(0.1 * rng.standard_normal((SLOTS, LAYERS, Nq + Nk, 8)), dt),
         "pos": rng.integers(0, T + 13, (ROWS, T)).astype(np.int32)}
    c["cos"], c["sin"] = rope_tables(T, hd)
    for v in c.values():
        v.setflags(write=False)
    return c


def run(case, dt, stages, slots, tiles, explicit_pos=True, args=None, expect_error=None):
    """one call on freshly uploaded buffers (La: the sentinel when stage A writes it, the given La when stage B runs alone); `tiles`: the
    per-tile entry point with `slots` [rows][nt], else the row-slot one with `slots` [rows].  Returns (La, qkv, prefilled La)"""
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    c = problem(case, dt)
    la0 = np.full((ROWS, T, 16), SENT, np.float32) if stages & A else c["La_in"]
    bf = Bufs(32 * max(ld, D))
    try:
        d = {k: bf.put(c[k], dt) for k in ("xn", "qkv", "bankA", "bankB")}
        d["La"] = bf.put(la0, dt)
        dslot = bf.put(np.asarray(slots, np.int32)) if slots is not None else None
        dcos, dsin = bf.put(c["cos"]), bf.put(c["sin"])
        dpos = bf.put(c["pos"]) if explicit_pos else None
        a = dict(rows=ROWS, Ttok=T, D=D, H=H, KV=KV, hd=hd, L=LAYERS, layer=LAYER)
        a.update(args or {})
        if tiles:
            rc = bf.L.rsys_op_adapter_bank_tiles(dt, stages, a["rows"], a["Ttok"], a["D"], a["H"], a["KV"], a["hd"], a["L"], a["layer"], dslot,
                                                 d["bankA"], d["bankB"], d["xn"], d["La"], d["qkv"], dcos, dsin, dpos, c["cos"].shape[0])
        else:
            rc = bf.L.rsys_op_adapter_bank(dt, stages, 0, a["rows"], a["Ttok"], a["D"], a["H"], a["KV"], a["hd"], a["L"], a["layer"], C.c_float(0.0), 0, 0,
                                           dslot, d["bankA"], d["bankB"], d["xn"], d["La"], d["qkv"], None, None, None, None, None, None, None,
                                           dcos, dsin, dpos, c["cos"].shape[0])
        if expect_error is None:
            assert rc == 0, _lib().last_error()
        else:
            assert rc != 0 and expect_error in _lib().last_error(), (rc, _lib().last_error())
        out = bf.get(d["La"], la0.shape, dt), bf.get(d["qkv"], c["qkv"].shape, dt), la0      # (get checks the sentinel tails)
        for k in ("xn", "bankA", "bankB"):
            assert same(bf.get(d[k], c[k].shape, dt), c[k]), k
        return out
    finally:
        bf.free()


@functools.lru_cache(maxsize=None)
def by_slot(case, dt, stages, explicit_pos):
    """the row-slot kernels with every row on slot s, for every slot the case's tile map names: computed once, shared, never modified"""
    out = {}
    for s in sorted(set(int(v) for v in tile_map(case).ravel()) - {-1}):
        la, qkv, _ = run(case, dt, stages, [s] * ROWS, False, explicit_pos)
        la.setflags(write=False); qkv.setflags(write=False)
        out[s] = (la, qkv)
    return out


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("stages", [A, B, A | B], ids=["a", "b", "ab"])
def test_tiles_equal_the_row_slot_kernels_tile_by_tile(case, dt, stages):
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    tm = tile_map(case)
    explicit = not (case == 4 and stages == B)            # one case on implicit positions (token t of a row at position t)
    la, qkv, la0 = run(case, dt, stages, tm, True, explicit)
    ref = by_slot(case, dt, stages, explicit)
    want_la, want_qkv = la0.copy(), problem(case, dt)["qkv"].copy()
    for r in range(ROWS):
        for j in range(tm.shape[1]):
            if tm[r, j] >= 0:
                t = slice(64 * j, min(64 * j + 64, T))
                want_la[r, t], want_qkv[r, t] = ref[int(tm[r, j])][0][r, t], ref[int(tm[r, j])][1][r, t]
    assert same(la, want_la)                              # (-1 tiles: the prefill, bit for bit)
    assert same(qkv, want_qkv)
    assert same(qkv[:, :, Nq:Nq + Nk], problem(case, dt)["qkv"][:, :, Nq:Nq + Nk])          # k columns unwritten
    if stages & B:                                        # the comparison is not vacuous: live tiles moved, and neighbours differ
        live = np.repeat(tm >= 0, 64, axis=1)[:, :T]
        moved = (qkv != problem(case, dt)["qkv"])[:, :, :Nq].any(axis=2)
        assert np.array_equal(moved, live)
    if stages == A | B and tm.shape[1] > 1:
        s0, s1 = int(tm[0, 0]), int(tm[0, -1])
        assert not same(ref[s0][1][0], ref[s1][1][0])


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_refusals_leave_the_outputs_unwritten(dt):
    case = 2
    tm = tile_map(case)
    c = problem(case, dt)

    def refused(err, stages=A | B, slots=tm, **args):
        la, qkv, la0 = run(case, dt, stages, slots, True, args=args or None, expect_error=err)
        assert same(la, la0) and same(qkv, c["qkv"])

    refused("stages 1 and 2 only", stages=4)
    refused("stages 1 and 2 only", stages=A | 64)
    refused("stages is a mask", stages=0)
    bad = tm.copy(); bad[2, 1] = 8
    refused("entries must be in [-1", slots=bad)
    bad = tm.copy(); bad[0, 0] = -2
    refused("entries must be in [-1", slots=bad)
    refused("is null", slots=None)
    refused("Ttok % 8", Ttok=68)
    refused("D must be H * hd", H=4)
    refused("layer outside", layer=LAYERS)
