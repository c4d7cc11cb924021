"""CPU: the float64 reference of the adapter bank's stages (tests/_adapter_bank_np.py) on its own: the composition of the per-stage
functions without rounding equals LoRA's forward and backward written directly, and the rounding points sit where adapter_bank.hip
documents them."""
import numpy as np

import _adapter_bank_np as ab

ROW_SLOT = [3, -1, 0, 3, 7]


def _problem(seed=5, rows=5, T=24, H=3, KV=1, hd=16, L=2, explicit_pos=True):
    rng = np.random.default_rng(seed)
    D, Nq, Nk = H * hd, H * hd, KV * hd
    ld = Nq + 2 * Nk
    c = dict(H=H, KV=KV, hd=hd)
    c["xn"] = rng.standard_normal((rows, T, D)); c["qkv"] = rng.standard_normal((rows, T, ld))
    c["dqkv"] = rng.standard_normal((rows, T, ld)); c["dxn"] = rng.standard_normal((rows, T, D))
    c["bankA"] = 0.1 * rng.standard_normal((8, L, 16, D)); c["bankB"] = 0.1 * rng.standard_normal((8, L, Nq + Nk, 8))
    c["gA"] = rng.standard_normal((8, L, 16, D)); c["gB"] = rng.standard_normal((8, L, Nq + Nk, 8))
    rope_rows = T + 9
    ang = np.outer(np.arange(rope_rows), 1.0 / 10000 ** (np.arange(hd // 2) / (hd // 2)))
    c["cos"], c["sin"] = np.cos(ang), np.sin(ang)
    c["pos"] = rng.integers(0, rope_rows, (rows, T)) if explicit_pos else None
    return c


def _chain(c, dt, mask=None, p=0.0):
    return ab.chain(dt, c["xn"], c["qkv"], c["dqkv"], c["dxn"], c["bankA"], c["bankB"], ROW_SLOT, 1, c["gA"], c["gB"], c["H"], c["KV"], c["hd"],
                    c["cos"], c["sin"], c["pos"], mask=mask, p=p)


def test_composition_equals_direct_lora():
    for explicit in (True, False):
        c = _problem(explicit_pos=explicit)
        o = _chain(c, None)
        q, dx, gA, gB = ab.lora_direct(c["xn"], c["qkv"], c["dqkv"], c["dxn"], c["bankA"], c["bankB"], ROW_SLOT, 1, c["gA"], c["gB"], c["H"],
                                       c["KV"], c["hd"], c["cos"], c["sin"], c["pos"])
        for name, a, b in (("qkv", o["qkv"], q), ("dxn", o["dxn"], dx), ("gA", o["gA"], gA), ("gB", o["gB"], gB)):
            assert np.allclose(a, b, rtol=1e-12, atol=1e-12), name
        Nq, Nk = c["H"] * c["hd"], c["KV"] * c["hd"]
        # what no stage may touch: the k columns, the slot -1 row, layer 0 and the slots without a row
        assert np.array_equal(o["qkv"][..., Nq:Nq + Nk], c["qkv"][..., Nq:Nq + Nk])
        assert np.array_equal(o["qkv"][1], c["qkv"][1]) and np.array_equal(o["dxn"][1], c["dxn"][1])
        assert np.array_equal(o["gA"][:, 0], c["gA"][:, 0]) and np.array_equal(o["gB"][[1, 2, 4, 5, 6]], c["gB"][[1, 2, 4, 5, 6]])
        assert not np.any(o["partA"][1]) and not np.any(o["partB"][1]) and not np.any(o["La"][1])


def test_mag_bounds_value():
    c = _problem(seed=9)
    o = _chain(c, None)
    for k in ("La", "dLa", "partA", "partB"):
        assert np.all(np.abs(o[k + "64"] if k + "64" in o else o[k]) <= o[k + "_mag"] * (1 + 1e-12))
    assert np.all(np.abs(o["qkv"]) <= o["qkv_mag"] * (1 + 1e-12) + np.abs(c["qkv"]) * (o["qkv_mag"] == 0))
    assert np.all(np.abs(o["gA"]) <= o["gA_mag"] * (1 + 1e-12)) and np.all(np.abs(o["gB"]) <= o["gB_mag"] * (1 + 1e-12))


def test_rounding_points():
    c = _problem(seed=11)
    for k in ("xn", "qkv", "dqkv", "dxn", "bankA", "bankB"):
        c[k] = ab.stored(c[k], ab.BF16)
    o = _chain(c, ab.BF16)
    # La and dLa are stored in the compute type
    assert np.array_equal(o["La"], ab.bf16_round(o["La"].astype(np.float32))) and not np.array_equal(o["La"], o["La64"])
    assert np.array_equal(o["dLa"], ab.bf16_round(o["dLa"].astype(np.float32)))
    # partB carries no factor 2: the reduction applies it
    red = sum(o["partB"][r] for r in (0, 3))
    assert np.allclose(o["gB"][3, 1] - c["gB"][3, 1], 2.0 * red, rtol=1e-12, atol=1e-12)
    assert np.allclose(o["gA"][3, 1] - c["gA"][3, 1], o["partA"][0] + o["partA"][3], rtol=1e-12, atol=1e-12)
    # dropout: the input is scaled, rounded and masked; dx is rounded to the compute type BEFORE the mask and the scale
    rng = np.random.default_rng(1)
    mask = (rng.random(c["xn"].shape) >= 0.25).astype(np.float64)
    od = _chain(c, ab.BF16, mask=mask, p=0.25)
    keep = ab.keep_of(0.25)
    assert np.array_equal(od["xd"], ab.stored(c["xn"] * keep, ab.BF16) * mask)
    assert np.array_equal(od["dxn"] - c["dxn"] == 0, (mask == 0) | (ab.stored(od["u"], ab.BF16) == 0) | (np.asarray(ROW_SLOT) < 0)[:, None, None])
    late = c["dxn"] + od["u"] * mask * keep
    assert not np.array_equal(od["dxn"], late) and np.all(np.abs(od["dxn"] - late) <= 2.0 ** -8 * np.abs(od["u"]) * keep * (1 + 1e-12))
    # the fp32 row reduction agrees with the fp64 one to fp32 accuracy and adds rows 0 then 3 for slot 3
    pa = o["partA"].astype(np.float32)
    g32 = ab.reduce32(pa, ROW_SLOT, c["gA"].astype(np.float32), 1, 1.0)
    assert np.array_equal(g32[3, 1], c["gA"].astype(np.float32)[3, 1] + (pa[0] + pa[3]))
    assert np.allclose(g32, o["gA"], rtol=1e-5, atol=1e-5)


def test_adamw_reference():
    rng = np.random.default_rng(2)
    n = 50
    p, g, m, v = rng.standard_normal(n), rng.standard_normal(n), 0.1 * rng.standard_normal(n), 0.01 * rng.random(n)
    norm, coef, p1, m1, v1 = ab.adamw(p, g, m, v, 1e-2, 0.9, 0.95, 1e-8, 0.1, 3, 1.0)
    assert abs(norm - np.linalg.norm(g)) < 1e-12 and abs(coef - 1.0 / (norm + 1e-6)) < 1e-12
    assert np.allclose(m1, 0.9 * m + 0.1 * g * coef, rtol=1e-6) and np.allclose(v1, 0.95 * v + 0.05 * (g * coef) ** 2, rtol=1e-6)
    _, coef0, _, _, _ = ab.adamw(p, g, m, v, 1e-2, 0.9, 0.95, 1e-8, 0.1, 3, 0.0)
    assert coef0 == 1.0
