"""float64 restatement of the adapter bank's stages on packed finetune rows (csrc/adapter_bank.hip) for
tests/test_gpu_adapter_bank_segments.py: tests/_adapter_bank_np.py's stages, composed over a segment table instead of one slot per row.
  - segs [n_seg][5] = (row, first column, columns, slot, task); a segment owns the whole 64-token tiles it touches, tokens
    [2 c0, min(T, 2 c0 + 64 ceil(columns / 32)));
  - the per-token stages (A, B, dLa, dx) take the slot of the token's tile: every token is handed to _adapter_bank_np as a row of its own
    (T = 1) with that slot, -1 where no segment owns the tile;
  - partA / partB [n_seg][..]: one partial per segment over its token range (_adapter_bank_np.da / db on that slice as one row);
  - the reduction sums a slot's partials over its segments in descriptor order (_adapter_bank_np.reduce / reduce32 with the segments'
    slots where the rows' slots were).
Layouts otherwise as _adapter_bank_np; positions are always explicit here ([rows][T])."""
import numpy as np

import _adapter_bank_np as ab


def token_range(seg, T):
    kb = 2 * int(seg[1])
    return kb, min(T, kb + 64 * (-(-int(seg[2]) // 32)))


def token_slot(segs, rows, T):
    """[rows][T]: the slot of the segment that owns the token's tile, -1 for a base-model segment or an unowned tile"""
    ts = np.full((rows, T), -1, np.int64)
    for sg in segs:
        kb, ke = token_range(sg, T)
        ts[int(sg[0]), kb:ke] = int(sg[3])
    return ts


def seg_slots(segs):
    return [int(sg[3]) for sg in segs]


def tok(x):
    """[rows][T][n] -> [rows * T][1][n]: every token a row of its own"""
    x = np.asarray(x)
    return x.reshape(-1, 1, x.shape[-1])


def per_segment(fn, segs, T, x, y, shape):
    """fn(x[row, kb:ke] as one row, y[...] as one row, [slot]) per segment -> (value [n_seg][..], mag); zeros for slot -1"""
    val, mag = np.zeros((len(segs),) + shape), np.zeros((len(segs),) + shape)
    for i, sg in enumerate(segs):
        if sg[3] < 0:
            continue
        kb, ke = token_range(sg, T)
        r = int(sg[0])
        v, m = fn(x[r:r + 1, kb:ke], y[r:r + 1, kb:ke], [int(sg[3])])
        val[i], mag[i] = v[0], m[0]
    return val, mag


def da(dLa, xd, segs):
    T, D = xd.shape[1], xd.shape[2]
    return per_segment(ab.da, segs, T, dLa, xd, (16, D))


def db(dqkv, La, segs, H, KV, hd):
    T = La.shape[1]
    return per_segment(lambda g, la, s: ab.db(g, la, s, H, KV, hd), segs, T, dqkv, La, ((H + KV) * hd, 8))


def chain(dt, xn, qkv, dqkv, dxn, bankA, bankB, segs, layer, gA, gB, H, KV, hd, cos, sin, pos):
    """all stages in production order with the rounding points applied; _adapter_bank_np.chain's keys (no dropout)"""
    rows, T, D = xn.shape
    ts = token_slot(segs, rows, T).ravel()
    back = lambda x: x.reshape(rows, T, x.shape[-1])
    p1 = np.asarray(pos).reshape(-1, 1)
    o = {"xd": np.asarray(xn, np.float64)}
    la, mag = ab.stage_a(tok(o["xd"]), bankA, ts, layer)
    o["La64"], o["La_mag"] = back(la), back(mag)
    o["La"] = ab.stored(o["La64"], dt)
    q, mag = ab.stage_b(tok(o["La"]), bankB, ts, layer, tok(qkv), H, KV, hd, cos, sin, p1)
    o["qkv"], o["qkv_mag"] = back(q), back(mag)
    g, mag = ab.dla(tok(dqkv), bankB, ts, layer, H, KV, hd)
    o["dLa64"], o["dLa_mag"] = back(g), back(mag)
    o["dLa"] = ab.stored(o["dLa64"], dt)
    o["partB"], o["partB_mag"] = db(np.asarray(dqkv, np.float64), o["La"], segs, H, KV, hd)
    o["partA"], o["partA_mag"] = da(o["dLa"], o["xd"], segs)
    u, mag = ab.dx_sum(tok(o["dLa"]), bankA, ts, layer)
    o["u"], o["u_mag"] = back(u), back(mag)
    o["dxn"] = ab.dx_finish(o["u"], np.asarray(dxn, np.float64), None, 0.0, dt)
    o["gA"], o["gA_mag"] = ab.reduce(o["partA"], seg_slots(segs), gA, layer, 1.0)
    o["gB"], o["gB_mag"] = ab.reduce(o["partB"], seg_slots(segs), gB, layer, 2.0)
    return o
