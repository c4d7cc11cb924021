"""float64 restatement of the adapter bank's stages (csrc/adapter_bank.hip) for tests/test_gpu_adapter_bank_ops.py, on storage-rounded
inputs.  Every stage returns (value, mag): the fp64 value and the sum of the magnitudes of the terms that went into it -- what a
rounding-count bound scales with.  The stages apply no rounding themselves; the rounding points adapter_bank.hip documents are separate
functions (stored(), dropped(), dx_finish(), reduce32()), which chain() applies where the kernels do:
  - La and dLa are stored in the compute type;
  - alpha = 2 multiplies the fp32 sum (stage B, dLa), a power of two: exact;
  - the q update is rotated, then added to the old value;
  - dx with p > 0 is rounded to the compute type before the mask and the scale;
  - partB does not carry the factor 2; the row reduction applies it.
Layouts: xn / dxn [rows][T][D], qkv / dqkv [rows][T][Nq + Nk + Nv], La / dLa [rows][T][16], bankA [slots][L][16][D], bankB
[slots][L][Nq + Nv][8], partA [rows][16][D], partB [rows][Nq + Nv][8], gA / gB in the banks' layouts.  A row with slot -1 is inactive: its
values are zeros here and must be left alone by the kernels."""
import numpy as np

F32, BF16 = 0, 1


def bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + ((u >> 16) & 1) + 0x7FFF) & 0xFFFF0000).view(np.float32)


def stored(x, dt):
    """the value a compute-type buffer holds for x, as float64 (dt None: no rounding)"""
    if dt is None:
        return np.asarray(x, np.float64)
    x32 = np.asarray(x, np.float64).astype(np.float32)
    return (bf16_round(x32) if dt == BF16 else x32).astype(np.float64)


def keep_of(p, dt=F32):
    """1 / (1 - p) as the kernels compute it (fp32)"""
    if dt is None:
        return 1.0 / (1.0 - p)
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def dropped(xn, mask, p, dt):
    """drop(xn): xn * keep under the mask, rounded to the compute type as launch_dropout stores it (mask None or p == 0: xn)"""
    if mask is None or p == 0:
        return np.asarray(xn, np.float64)
    return stored(np.asarray(xn, np.float64) * keep_of(p, dt), dt) * mask


def _act(row_slot):
    s = np.asarray(row_slot)
    return s >= 0, np.where(s >= 0, s, 0)


def stage_a(xd, bankA, row_slot, layer):
    """La[r, t, j] = sum_d xd[r, t, d] A[slot r][layer][j][d]"""
    act, s = _act(row_slot)
    A = bankA[s, layer] * act[:, None, None]
    return np.einsum("rtd,rjd->rtj", xd, A), np.einsum("rtd,rjd->rtj", np.abs(xd), np.abs(A))


def _rope_tables(cos, sin, pos, rows, T, H):
    """cos / sin per (row, token, pair of a q column): [rows][T][Nq / 2]"""
    if pos is None:
        pos = np.tile(np.arange(T), (rows, 1))
    pos = np.asarray(pos).reshape(rows, T)
    return np.tile(cos[pos], (1, 1, H)), np.tile(sin[pos], (1, 1, H))


def stage_b_update(La, bankB, row_slot, layer, H, KV, hd, cos, sin, pos, absolute=False):
    """(the rotated q update, the v update) = (rope(2 La[:, :8] . B_q^T), 2 La[:, 8:] . B_v^T); absolute: the same sums over magnitudes
    (the update's mag, and the sensitivity of the update to an error |dLa| in its input)"""
    rows, T, _ = La.shape
    Nq = H * hd
    act, s = _act(row_slot)
    B = bankB[s, layer] * act[:, None, None]
    if absolute:
        La, B = np.abs(La), np.abs(B)
    uq = 2.0 * np.einsum("rtk,rck->rtc", La[..., :8], B[:, :Nq])
    uv = 2.0 * np.einsum("rtk,rck->rtc", La[..., 8:], B[:, Nq:])
    cm, sm = _rope_tables(np.asarray(cos, np.float64), np.asarray(sin, np.float64), pos, rows, T, H)
    u0, u1 = uq[..., 0::2], uq[..., 1::2]
    rq = np.empty_like(uq)
    if absolute:
        cm, sm = np.abs(cm), np.abs(sm)
        rq[..., 0::2] = u0 * cm + u1 * sm
    else:
        rq[..., 0::2] = u0 * cm - u1 * sm
    rq[..., 1::2] = u0 * sm + u1 * cm
    return rq, uv


def stage_b(La, bankB, row_slot, layer, qkv, H, KV, hd, cos, sin, pos):
    """qkv with q += rope(2 La_q . B_q^T), v += 2 La_v . B_v^T; k as it was.  mag has qkv's shape (zeros in the k columns)"""
    Nq, Nk = H * hd, KV * hd
    rq, uv = stage_b_update(La, bankB, row_slot, layer, H, KV, hd, cos, sin, pos)
    mq, mv = stage_b_update(La, bankB, row_slot, layer, H, KV, hd, cos, sin, pos, absolute=True)
    act, _ = _act(row_slot)
    a3 = act[:, None, None]
    out = np.array(qkv, np.float64)
    mag = np.zeros_like(out)
    out[..., :Nq] += rq; out[..., Nq + Nk:] += uv
    mag[..., :Nq] = (mq + np.abs(qkv[..., :Nq])) * a3; mag[..., Nq + Nk:] = (mv + np.abs(qkv[..., Nq + Nk:])) * a3
    return out, mag


def dla(dqkv, bankB, row_slot, layer, H, KV, hd, absolute=False):
    """dLa[r, t, :8] = 2 dq . B_q, dLa[r, t, 8:] = 2 dv . B_v"""
    Nq, Nk = H * hd, KV * hd
    act, s = _act(row_slot)
    B = bankB[s, layer] * act[:, None, None]

    def f(g, B):
        return np.concatenate([2.0 * np.einsum("rtc,rck->rtk", g[..., :Nq], B[:, :Nq]),
                               2.0 * np.einsum("rtc,rck->rtk", g[..., Nq + Nk:], B[:, Nq:])], -1)
    return f(dqkv, B), f(np.abs(dqkv), np.abs(B))


def dx_sum(dLa_, bankA, row_slot, layer):
    """u[r, t, d] = sum_j dLa[r, t, j] A[slot r][layer][j][d], before dx_finish"""
    act, s = _act(row_slot)
    A = bankA[s, layer] * act[:, None, None]
    return np.einsum("rtj,rjd->rtd", dLa_, A), np.einsum("rtj,rjd->rtd", np.abs(dLa_), np.abs(A))


def dx_finish(u, old, mask, p, dt):
    """dxn = old + u, or with dropout old + stored(u) * mask * keep"""
    if mask is None or p == 0:
        return old + u
    return old + stored(u, dt) * mask * keep_of(p, dt)


def da(dLa_, xd, row_slot):
    """partA[r, j, d] = sum_t dLa[r, t, j] xd[r, t, d]"""
    act, _ = _act(row_slot)
    a3 = act[:, None, None]
    return np.einsum("rtj,rtd->rjd", dLa_, xd) * a3, np.einsum("rtj,rtd->rjd", np.abs(dLa_), np.abs(xd)) * a3


def db(dqkv, La, row_slot, H, KV, hd):
    """partB[r, c, j] = sum_t dq[r, t, c] La[r, t, j] (q columns), sum_t dv[r, t, c - Nq] La[r, t, 8 + j] (v columns); no factor 2"""
    Nq, Nk = H * hd, KV * hd
    act, _ = _act(row_slot)
    a3 = act[:, None, None]

    def f(g, La):
        return np.concatenate([np.einsum("rtc,rtj->rcj", g[..., :Nq], La[..., :8]), np.einsum("rtc,rtj->rcj", g[..., Nq + Nk:], La[..., 8:])], 1)
    return f(dqkv, La) * a3, f(np.abs(dqkv), np.abs(La)) * a3


def reduce(part, row_slot, g, layer, alpha):
    """g[slot][layer] += alpha * (sum of part[r] over the rows of the slot); mag = |g| + alpha sum |part[r]|"""
    out = np.array(g, np.float64)
    mag = np.abs(out)
    for a in sorted(set(int(s) for s in row_slot if s >= 0)):
        rs = [r for r, s in enumerate(row_slot) if s == a]
        out[a, layer] += alpha * sum(np.asarray(part[r], np.float64) for r in rs)
        mag[a, layer] += alpha * sum(np.abs(np.asarray(part[r], np.float64)) for r in rs)
    return out, mag


def reduce32(part, row_slot, g, layer, alpha):
    """the row reduction in the kernel's own fp32 order: the rows of a slot added in row order from 0, times alpha (exact), added to g"""
    out = np.array(g, np.float32)
    for a in sorted(set(int(s) for s in row_slot if s >= 0)):
        acc = np.zeros(part[0].shape, np.float32)
        for r, s in enumerate(row_slot):
            if s == a:
                acc = acc + np.asarray(part[r], np.float32)
        out[a, layer] = out[a, layer] + np.float32(alpha) * acc
    return out


def chain(dt, xn, qkv, dqkv, dxn, bankA, bankB, row_slot, layer, gA, gB, H, KV, hd, cos, sin, pos, mask=None, p=0.0):
    """all stages in production order with the rounding points applied (dt None: none); a dict of every intermediate and output"""
    o = {}
    o["xd"] = dropped(xn, mask, p, dt)
    o["La64"], o["La_mag"] = stage_a(o["xd"], bankA, row_slot, layer)
    o["La"] = stored(o["La64"], dt)
    o["qkv"], o["qkv_mag"] = stage_b(o["La"], bankB, row_slot, layer, qkv, H, KV, hd, cos, sin, pos)
    o["dLa64"], o["dLa_mag"] = dla(dqkv, bankB, row_slot, layer, H, KV, hd)
    o["dLa"] = stored(o["dLa64"], dt)
    o["partB"], o["partB_mag"] = db(dqkv, o["La"], row_slot, H, KV, hd)
    o["partA"], o["partA_mag"] = da(o["dLa"], o["xd"], row_slot)
    o["u"], o["u_mag"] = dx_sum(o["dLa"], bankA, row_slot, layer)
    o["dxn"] = dx_finish(o["u"], np.asarray(dxn, np.float64), mask, p, dt)
    o["gA"], o["gA_mag"] = reduce(o["partA"], row_slot, gA, layer, 1.0)
    o["gB"], o["gB_mag"] = reduce(o["partB"], row_slot, gB, layer, 2.0)
    return o


def lora_direct(xn, qkv, dqkv, dxn, bankA, bankB, row_slot, layer, gA, gB, H, KV, hd, cos, sin, pos):
    """LoRA forward and backward written directly (model.py:235-271 with lora_scaling 2), one row at a time: q += rope(2 (x A_q^T) B_q^T),
    v += 2 (x A_v^T) B_v^T; dA = (2 g B)^T x, dB = 2 g^T (x A^T), dx += (2 g_q B_q) A_q + (2 g_v B_v) A_v, summed per slot"""
    rows, T, D = xn.shape
    Nq, Nk = H * hd, KV * hd
    q_out = np.array(qkv, np.float64); dx_out = np.array(dxn, np.float64)
    gA_out = np.array(gA, np.float64); gB_out = np.array(gB, np.float64)
    cm, sm = _rope_tables(np.asarray(cos, np.float64), np.asarray(sin, np.float64), pos, rows, T, H)
    for r, s in enumerate(row_slot):
        if s < 0:
            continue
        Aq, Av = bankA[s, layer, :8], bankA[s, layer, 8:]
        Bq, Bv = bankB[s, layer, :Nq], bankB[s, layer, Nq:]
        x = xn[r]
        uq = 2.0 * np.einsum("td,kd,ck->tc", x, Aq, Bq)
        uv = 2.0 * np.einsum("td,kd,ck->tc", x, Av, Bv)
        rot = np.empty_like(uq)
        rot[:, 0::2] = uq[:, 0::2] * cm[r] - uq[:, 1::2] * sm[r]
        rot[:, 1::2] = uq[:, 0::2] * sm[r] + uq[:, 1::2] * cm[r]
        q_out[r, :, :Nq] += rot; q_out[r, :, Nq + Nk:] += uv
        gq, gv = dqkv[r, :, :Nq], dqkv[r, :, Nq + Nk:]
        gA_out[s, layer, :8] += 2.0 * np.einsum("tc,ck,td->kd", gq, Bq, x)
        gA_out[s, layer, 8:] += 2.0 * np.einsum("tc,ck,td->kd", gv, Bv, x)
        gB_out[s, layer, :Nq] += 2.0 * np.einsum("tc,td,kd->ck", gq, x, Aq)
        gB_out[s, layer, Nq:] += 2.0 * np.einsum("tc,td,kd->ck", gv, x, Av)
        dx_out[r] += 2.0 * (np.einsum("tc,ck,kd->td", gq, Bq, Aq) + np.einsum("tc,ck,kd->td", gv, Bv, Av))
    return q_out, dx_out, gA_out, gB_out


def adamw(p, g, m, v, lr, b1, b2, eps, wd, step, max_norm):
    """the bank's per-slot clip + AdamW in fp64 (fp32 hyper-parameters): returns norm, new p, m, v"""
    f = lambda a: float(np.float32(a))
    lr, b1, b2, eps, wd, max_norm = f(lr), f(b1), f(b2), f(eps), f(wd), f(max_norm)
    g = np.asarray(g, np.float64)
    norm = float(np.sqrt((g * g).sum()))
    coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    gk = g * coef
    m1 = b1 * m + (1 - b1) * gk
    v1 = b2 * v + (1 - b2) * gk * gk
    bc1 = 1 - b1 ** step; bc2s = np.sqrt(1 - b2 ** step)
    p1 = p * (1 - lr * wd) - (lr / bc1) * (m1 / (np.sqrt(v1) / bc2s + eps))
    return norm, coef, p1, m1, v1
