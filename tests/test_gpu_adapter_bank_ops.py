"""GPU: the adapter bank's kernels (csrc/adapter_bank.hip), one launch at a time and all together, through rsys_op_adapter_bank /
rsys_op_adapter_bank_adamw / rsys_op_dropout (rsys_debug.h) against the float64 reference of tests/_adapter_bank_np.py on the same
storage-rounded inputs.  The shapes are the smallest that reach every ragged branch of the kernels (checked against the code):

  case  Ttok  D   H KV hd   what it reaches
  1       8   16  1 1  16   one half token tile (tok_ok false on 8 lanes); D = 16: one K step, waves 1-3 idle in stage A (fp32 and bf16), and
                            that bf16 step is ragged (k_ok false for kq >= 2); dLa: bf16 sq + sv = 2, fp32 2 steps: idle waves; KV == H
  2      24   48  3 1  16   Ttok % 16 == 8 with a full tile before it; fp32 dA / dB: a ragged last token-K step (24 % 16); bf16 dLa: Nq = 48 and
                            Nv = 16 both end in a ragged step, sq + sv = 3 < 4; bf16 dA / dB: one ragged step (24 < 32)
  3      40   80  5 5  16   bf16 dA / dB: 40 % 32 == 8, a ragged second step; D = 80: dA's second workgroup has three idle waves; fp32 stage A: 5 K
                            steps, wave 0 runs a second round; Nq + Nv = 160: dB's third workgroup is half idle; bf16 stage A: ragged third step
  4      72  160  5 1  32   hd 32; Ttok 72 = the trimmed row_len 36 (a half tile after four full ones); bf16 stage A: 5 steps, wave 0 runs a second
                            round; fp32 stage A: 10 steps, 3 rounds; dLa: fp32 12 steps, 3 rounds; bf16 5 + 1 steps, all whole (8 | hd and hd >= 16
                            make every fp32 dLa step whole at any legal shape; a bf16 one is ragged only with hd 16, cases 1 - 3)
  5     136  320  5 5  64   stage B: 8 tokens x 80 items > 256 and dx: 8 x 40 > 256 loop; 17 token tiles of 8, 9 of 16 (the last half full)
  6      48  256  2 1 128   hd 128
  7     128  128  2 1  64   the regular shape of the whole-model tests (control)

Fixed: rows = 5, L = 2, layer = 1 (a non-zero layer offset), row_slot = [3, -1, 0, 3, 7] (the last slot; one slot on two rows that are not
neighbours; one row without an adapter, which must stay bit for bit).

Bounds are derived, not tuned (u = 2^-24).  |got - ref| <= (c + 1) u sum|terms| for a value the kernel holds in fp32, c = the roundings on
the longest chain of the kernel's summation order and + 1 for the terms of second order; a bf16-stored value gets one bf16 ulp of the
reference on top.  An MFMA step over k contraction elements counts as k roundings in bf16 (exact products, every addition may round) and
2 k in fp32 (the product may round too): nothing narrower is documented for the instruction.  Factors of 2 are exact and count 0.
  stage A   R KS ceil(ceil(D / KS) / 4) (a wave's K rounds) + 3 (cross-wave adds);  R = 1, KS = 32 (bf16) or R = 2, KS = 16 (fp32)
  dLa       R KS ceil((sq + sv) / 4) + 3
  stage B   8 (fma chain) + 2 (rotation: product, sum) + 1 (+ old) = 11 on q; 8 + 1 = 9 on v
  dx        16 (fma chain) + 1 (+ old) = 17; with dropout 16, the compute-type rounding (reference: the same point), 1 (x keep), 1 (+ old)
  dA / dB   R KS ceil(Ttok / KS): one wave owns the whole contraction
  reduce    1 (rows 0 + 3; a single row adds to zero exactly) + 1 (+ g) = 2, and bit-equal to the same two additions in numpy fp32
Each check prints the largest error as a fraction of its bound (`pytest -s`)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import _adapter_bank_np as ab
from test_gpu_row_kernels import ADAM, BF16, F32, SENT, U, _adamw_ref, _lib, bf16_round, bf16_ulp, storage

pytestmark = pytest.mark.gpu

DTYPES = [F32, BF16]
ROWS, LAYERS, LAYER, SLOTS = 5, 2, 1, 8
ROW_SLOT = [3, -1, 0, 3, 7]
ACTIVE = [r for r, s in enumerate(ROW_SLOT) if s >= 0]
CASES = {1: (8, 16, 1, 1, 16), 2: (24, 48, 3, 1, 16), 3: (40, 80, 5, 5, 16), 4: (72, 160, 5, 1, 32), 5: (136, 320, 5, 5, 64),
         6: (48, 256, 2, 1, 128), 7: (128, 128, 2, 1, 64)}
A, B, DLA, DB, DA, DX, RED, ALL = 1, 2, 4, 8, 16, 32, 64, 127
OUTPUTS = ("La", "qkv", "dLa", "dxn", "partA", "partB", "gA", "gB")
FP32_BUFS = ("partA", "partB", "gA", "gB")
RATIO = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


class Bufs:
    """device buffers of one call; every buffer has a sentinel tail of `guard` elements (32 token rows of the widest array: a kernel that
    ignores a ragged-edge predicate stays inside an allocation, and shows)"""

    def __init__(self, guard):
        self.L = _lib().lib()
        self.guard = guard
        self.ptrs = []

    def put(self, arr, dt=F32):
        a = np.asarray(arr)
        if a.dtype.kind in "iu":
            h = np.concatenate([a.ravel().astype(np.int32), np.zeros(self.guard, np.int32)])
        elif dt == BF16:
            h = np.concatenate([bits(bf16_round(a.ravel())) >> 16, np.full(self.guard, 0xC0F0, np.uint32)]).astype(np.uint16)
        else:
            h = np.concatenate([a.ravel().astype(np.float32), np.full(self.guard, SENT, np.float32)])
        p = C.c_void_p()
        assert self.L.rsys_dev_alloc(C.byref(p), h.nbytes) == 0, _lib().last_error()
        self.ptrs.append(p)
        assert self.L.rsys_dev_h2d(p, h.ctypes.data, h.nbytes) == 0
        return p

    def get(self, p, shape, dt=F32):
        n = int(np.prod(shape))
        h = np.empty(n + self.guard, np.uint16 if dt == BF16 else np.float32)
        assert self.L.rsys_dev_d2h(h.ctypes.data, p, h.nbytes) == 0
        if dt == BF16:
            h = (h.astype(np.uint32) << 16).view(np.float32)
        assert np.all(h[n:] == SENT), "write past the end of the buffer"
        return h[:n].reshape(shape)

    def free(self):
        for p in self.ptrs:
            self.L.rsys_dev_free(p)
        self.ptrs = []


def dims(case):
    T, D, H, KV, hd = CASES[case]
    Nq, Nk = H * hd, KV * hd
    return T, D, H, KV, hd, Nq, Nk, Nq + 2 * Nk


def rope_tables(T, hd):
    rope_rows = T + 13
    ang = np.outer(np.arange(rope_rows), 1.0 / 10000.0 ** (np.arange(hd // 2) / (hd // 2)))
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


@functools.lru_cache(maxsize=None)
def problem(case, dt, variant=0):
    """storage-rounded host arrays of one case; variant 1 replaces the data of the rows that do not name slot 3"""
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    rng = np.random.default_rng(100 * case + dt)
    c = {}
    c["xn"] = storage(rng.standard_normal((ROWS, T, D)), dt)
    c["qkv"] = storage(rng.standard_normal((ROWS, T, ld)), dt)
    c["dqkv"] = storage(0.5 * rng.standard_normal((ROWS, T, ld)), dt)
    c["dxn"] = storage(rng.standard_normal((ROWS, T, D)), dt)
    c["bankA"] = storage(0.1 * rng.standard_normal((SLOTS, LAYERS, 16, D)), dt)
    c["bankB"] = storage(0.1 * rng.standard_normal((SLOTS, LAYERS, Nq + Nk, 8)), dt)
    c["gA"] = rng.standard_normal((SLOTS, LAYERS, 16, D)).astype(np.float32)
    c["gB"] = rng.standard_normal((SLOTS, LAYERS, Nq + Nk, 8)).astype(np.float32)
    c["cos"], c["sin"] = rope_tables(T, hd)
    c["pos"] = rng.integers(0, T + 13, (ROWS, T)).astype(np.int32)
    if variant:
        r2 = np.random.default_rng(7)
        for r in (1, 2, 4):
            for k in ("xn", "qkv", "dqkv", "dxn"):
                c[k] = c[k].copy()
                c[k][r] = storage(r2.standard_normal(c[k][r].shape), dt)
    for k, v in c.items():
        v.setflags(write=False)
    return c


def f64(c, *names):
    return [np.asarray(c[n], np.float64) for n in names]


@functools.lru_cache(maxsize=None)
def reference(case, dt, variant=0):
    """the fp64 chain with the rounding points applied (explicit positions); shared by the tests, never modified"""
    c = problem(case, dt, variant)
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    xn, qkv, dqkv, dxn, bankA, bankB, gA, gB = f64(c, "xn", "qkv", "dqkv", "dxn", "bankA", "bankB", "gA", "gB")
    return ab.chain(dt, xn, qkv, dqkv, dxn, bankA, bankB, ROW_SLOT, LAYER, gA, gB, H, KV, hd, c["cos"], c["sin"], c["pos"])


def prefill(case, dt, c, over=None):
    """the host image of every buffer before a call: inputs from the problem, pure outputs full of the sentinel"""
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    h = {k: c[k] for k in ("xn", "qkv", "dqkv", "dxn", "bankA", "bankB", "gA", "gB")}
    h["La"] = np.full((ROWS, T, 16), SENT, np.float32); h["dLa"] = np.full((ROWS, T, 16), SENT, np.float32)
    h["partA"] = np.full((ROWS, 16, D), SENT, np.float32); h["partB"] = np.full((ROWS, Nq + Nk, 8), SENT, np.float32)
    if over:
        for k, v in over.items():
            h[k] = storage(v, F32 if k in FP32_BUFS else dt)
    return h


def run(case, dt, c, stages, over=None, train=0, p=0.0, seed=0, stream=0, explicit_pos=True, args=None, row_slot=None, pos=None,
        rope_rows=None, expect_error=None):
    """one rsys_op_adapter_bank call on freshly uploaded buffers; returns every output buffer (guard tails checked).  args: overrides of the
    scalar arguments (ARG-error tests)"""
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    h = prefill(case, dt, c, over)
    bf = Bufs(32 * max(ld, D))
    try:
        d = {k: bf.put(v, F32 if k in FP32_BUFS else dt) for k, v in h.items()}
        dslot = bf.put(np.asarray(ROW_SLOT if row_slot is None else row_slot, np.int32))
        dcos, dsin = bf.put(c["cos"]), bf.put(c["sin"])
        pos = c["pos"] if pos is None else pos
        dpos = bf.put(pos) if explicit_pos else None
        a = dict(rows=ROWS, Ttok=T, D=D, H=H, KV=KV, hd=hd, L=LAYERS, layer=LAYER)
        a.update(args or {})
        rc = bf.L.rsys_op_adapter_bank(dt, stages, train, a["rows"], a["Ttok"], a["D"], a["H"], a["KV"], a["hd"], a["L"], a["layer"], C.c_float(p),
                                       seed, stream, dslot, d["bankA"], d["bankB"], d["xn"], d["La"], d["qkv"], d["dqkv"], d["dLa"], d["dxn"],
                                       d["partA"], d["partB"], d["gA"], d["gB"], dcos, dsin, dpos,
                                       c["cos"].shape[0] if rope_rows is None else rope_rows)
        if expect_error is None:
            assert rc == 0, _lib().last_error()
        else:
            assert rc != 0 and expect_error in _lib().last_error(), (rc, _lib().last_error())
        out = {k: bf.get(d[k], h[k].shape, F32 if k in FP32_BUFS else dt) for k in OUTPUTS}
        for k in ("xn", "dqkv", "bankA", "bankB"):   # inputs are read only
            assert same(bf.get(d[k], h[k].shape, dt), h[k]), k
        out["prefill"] = h
        return out
    finally:
        bf.free()


def check(kernel, dt, got, ref, bound, t_stored, what=""):
    """|got - ref| <= bound (+ one bf16 ulp of ref for a bf16-stored value); prints the worst error as a fraction of the bound"""
    tol = bound + (bf16_ulp(ref) if (t_stored and dt == BF16) else 0.0)
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(tol > 0), (kernel, "a zero bound")
    r = float((err / tol).max())
    key = (kernel, "bf16" if dt == BF16 else "fp32")
    RATIO[key] = max(RATIO.get(key, 0.0), r)
    print(f"ratio {key[0]} {key[1]} {what}: max err / bound = {r:.3f} (worst so far {RATIO[key]:.3f})")
    assert r <= 1.0, (kernel, what, r, np.unravel_index(np.argmax(err / tol), err.shape))


def mfma(dt):
    return (1, 32) if dt == BF16 else (2, 16)   # (roundings per contraction element, K per step)


def c_stage_a(D, dt):
    R, KS = mfma(dt)
    return R * KS * math.ceil(math.ceil(D / KS) / 4) + 3


def c_dla(Nq, Nv, dt):
    R, KS = mfma(dt)
    return R * KS * math.ceil((math.ceil(Nq / KS) + math.ceil(Nv / KS)) / 4) + 3


def c_tokens(T, dt):
    R, KS = mfma(dt)
    return R * KS * math.ceil(T / KS)


def b_bound(case, mag):
    """stage B: 11 roundings on the q columns, 9 on the v columns"""
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    cnt = np.zeros(ld); cnt[:Nq] = 11 + 1; cnt[Nq + Nk:] = 9 + 1
    return cnt * U * mag


def qv_cols(case):
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    return np.r_[0:Nq, Nq + Nk:ld], np.r_[Nq:Nq + Nk]


def untouched(case, out, stages, p=0.0):
    """everything a call must leave bit for bit: what no selected stage writes, and in the written buffers the slot -1 row, the k columns,
    layer 0 and the slots without a row (the rows after a half tile are the next batch row's: row 1 after row 0 is the slot -1 row)"""
    h = out["prefill"]
    qv, kc = qv_cols(case)
    writes = {"La": A, "qkv": B, "dLa": DLA, "dxn": DX, "partA": DA, "partB": DB, "gA": RED, "gB": RED}
    for k in OUTPUTS:
        if not stages & writes[k]:
            assert same(out[k], h[k]), (k, "written by a stage that was not selected")
        elif k in ("gA", "gB"):
            assert same(out[k][:, 0], h[k][:, 0]), (k, "layer 0")
            assert same(out[k][[1, 2, 4, 5, 6]], h[k][[1, 2, 4, 5, 6]]), (k, "slots without a row")
        else:
            assert same(out[k][1], h[k][1]), (k, "the slot -1 row")
    if stages & B:
        assert same(out["qkv"][..., kc], h["qkv"][..., kc]), "k columns"


# ============================================================================================ every stage alone
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("dt", DTYPES)
def test_stages_alone(case, dt):
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    c, o = problem(case, dt), reference(case, dt)
    act = ACTIVE
    qv, kc = qv_cols(case)
    what = f"case {case}"
    # ---- stage A, the inference kernel (DROP = false); the training one (DROP = true) at p = 0 must give the same bits
    out = run(case, dt, c, A)
    untouched(case, out, A)
    check("a", dt, out["La"][act], o["La64"][act], (c_stage_a(D, dt) + 1) * U * o["La_mag"][act], True, what)
    out_t = run(case, dt, c, A, train=1, p=0.0, seed=11, stream=70)
    assert same(out_t["La"], out["La"]), "a_train at p = 0 differs from the inference stage A"
    # ---- stage B on the stored reference La: explicit positions, then token t at position t
    for explicit in (True, False):
        xq, xm = ab.stage_b(o["La"], np.asarray(c["bankB"], np.float64), ROW_SLOT, LAYER, np.asarray(c["qkv"], np.float64), H, KV, hd, c["cos"],
                            c["sin"], c["pos"] if explicit else None)
        out = run(case, dt, c, B, over={"La": o["La"]}, explicit_pos=explicit)
        untouched(case, out, B)
        check("b", dt, out["qkv"][act][..., qv], xq[act][..., qv], b_bound(case, xm)[act][..., qv], True, f"{what} explicit {explicit}")
    # ---- dLa
    out = run(case, dt, c, DLA)
    untouched(case, out, DLA)
    check("dla", dt, out["dLa"][act], o["dLa64"][act], (c_dla(Nq, Nk, dt) + 1) * U * o["dLa_mag"][act], True, what)
    # ---- dB partials on the stored La, dA partials on the stored dLa (fp32 outputs)
    out = run(case, dt, c, DB, over={"La": o["La"]})
    untouched(case, out, DB)
    check("db", dt, out["partB"][act], o["partB"][act], (c_tokens(T, dt) + 1) * U * o["partB_mag"][act], False, what)
    out = run(case, dt, c, DA, over={"dLa": o["dLa"]})
    untouched(case, out, DA)
    check("da", dt, out["partA"][act], o["partA"][act], (c_tokens(T, dt) + 1) * U * o["partA_mag"][act], False, what)
    # ---- dx on the stored dLa, added to the old dxn
    out = run(case, dt, c, DX, over={"dLa": o["dLa"]})
    untouched(case, out, DX)
    check("dx", dt, out["dxn"][act], o["dxn"][act], (17 + 1) * U * (o["u_mag"] + np.abs(c["dxn"]))[act], True, what)
    # ---- the row reductions on the reference partials (as fp32): added to the prefilled gA / gB; slot 3 = rows 0 then 3 in fp32, bit for bit
    pa, pb = o["partA"].astype(np.float32), o["partB"].astype(np.float32)
    out = run(case, dt, c, RED, over={"partA": pa, "partB": pb})
    untouched(case, out, RED)
    assert same(out["gA"], ab.reduce32(pa, ROW_SLOT, c["gA"], LAYER, 1.0)) and same(out["gB"], ab.reduce32(pb, ROW_SLOT, c["gB"], LAYER, 2.0))
    for name, part, alpha in (("gA", pa, 1.0), ("gB", pb, 2.0)):
        ref, mag = ab.reduce(part.astype(np.float64), ROW_SLOT, np.asarray(c[name], np.float64), LAYER, alpha)
        check("reduce", dt, out[name][[0, 3, 7], LAYER], ref[[0, 3, 7], LAYER], (2 + 1) * U * mag[[0, 3, 7], LAYER], False, f"{what} {name}")
        assert not same(out[name][[0, 3, 7], LAYER], c[name][[0, 3, 7], LAYER])


# ============================================================================================ all stages in one call
def allowances(case, dt, c, o):
    """How far the one-call outputs may be from the fp64 chain: every stage's own bound, plus the reference's sensitivity to the stored
    inputs that stage read -- the stage's linear map applied to the magnitudes of the upstream allowance (all maps here are linear in the
    intermediate).  dLa_err / La_err: the bound of the stage that made it, + one bf16 ulp for the stored rounding (two values within the
    bound of each other can round one ulp apart)."""
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    ulp = (lambda x: bf16_ulp(x)) if dt == BF16 else (lambda x: 0.0)
    bankA, bankB, dqkv = f64(c, "bankA", "bankB", "dqkv")
    La_err = (c_stage_a(D, dt) + 1) * U * o["La_mag"] + ulp(o["La64"])
    dLa_err = (c_dla(Nq, Nk, dt) + 1) * U * o["dLa_mag"] + ulp(o["dLa64"])
    sq, sv = ab.stage_b_update(La_err, bankB, ROW_SLOT, LAYER, H, KV, hd, c["cos"], c["sin"], c["pos"], absolute=True)
    al = {}
    al["qkv"] = b_bound(case, o["qkv_mag"])
    al["qkv"][..., :Nq] += sq; al["qkv"][..., Nq + Nk:] += sv
    al["dxn"] = (17 + 1) * U * (o["u_mag"] + np.abs(c["dxn"])) + ab.dx_sum(dLa_err, bankA, ROW_SLOT, LAYER)[1]
    partA_err = (c_tokens(T, dt) + 1) * U * o["partA_mag"] + ab.da(dLa_err, o["xd"], ROW_SLOT)[1]
    partB_err = (c_tokens(T, dt) + 1) * U * o["partB_mag"] + ab.db(dqkv, La_err, ROW_SLOT, H, KV, hd)[1]
    zA, zB = np.zeros_like(o["gA"]), np.zeros_like(o["gB"])
    al["gA"] = (2 + 1) * U * o["gA_mag"] + ab.reduce(partA_err, ROW_SLOT, zA, LAYER, 1.0)[0]
    al["gB"] = (2 + 1) * U * o["gB_mag"] + ab.reduce(partB_err, ROW_SLOT, zB, LAYER, 2.0)[0]
    return al


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("dt", DTYPES)
def test_all_stages(case, dt):
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    c, o = problem(case, dt), reference(case, dt)
    act = ACTIVE
    qv, kc = qv_cols(case)
    what = f"case {case}"
    out = run(case, dt, c, ALL, train=1)
    untouched(case, out, ALL)
    # loss-free: each intermediate equals the single-stage run fed the same stored intermediates, bit for bit
    assert same(out["La"], run(case, dt, c, A, train=1)["La"])
    assert same(out["dLa"], run(case, dt, c, DLA)["dLa"])
    assert same(out["partB"], run(case, dt, c, DB, over={"La": out["La"]})["partB"])
    assert same(out["partA"], run(case, dt, c, DA, over={"dLa": out["dLa"]})["partA"])
    # end to end against the fp64 chain
    al = allowances(case, dt, c, o)
    check("all.qkv", dt, out["qkv"][act][..., qv], o["qkv"][act][..., qv], al["qkv"][act][..., qv], True, what)
    check("all.dxn", dt, out["dxn"][act], o["dxn"][act], al["dxn"][act], True, what)
    check("all.gA", dt, out["gA"][[0, 3, 7], LAYER], o["gA"][[0, 3, 7], LAYER], al["gA"][[0, 3, 7], LAYER], False, what)
    check("all.gB", dt, out["gB"][[0, 3, 7], LAYER], o["gB"][[0, 3, 7], LAYER], al["gB"][[0, 3, 7], LAYER], False, what)
    # accumulation: slot 3's gradient is its prefill plus the partials of rows 0 and 3, added in row order in fp32
    assert same(out["gA"], ab.reduce32(out["partA"], ROW_SLOT, c["gA"], LAYER, 1.0))
    assert same(out["gB"], ab.reduce32(out["partB"], ROW_SLOT, c["gB"], LAYER, 2.0))
    # reproducible: the same call again gives the same bits
    again = run(case, dt, c, ALL, train=1)
    for k in OUTPUTS:
        assert same(out[k], again[k]), k
    # independent: other data in the rows that do not name slot 3 leaves slot 3's gradients, and its rows' outputs, bit for bit
    other = run(case, dt, problem(case, dt, 1), ALL, train=1)
    assert same(other["gA"][3], out["gA"][3]) and same(other["gB"][3], out["gB"][3])
    for k in ("La", "qkv", "dLa", "dxn", "partA", "partB"):
        assert same(other[k][[0, 3]], out[k][[0, 3]]), k
    assert not same(other["gA"][0], out["gA"][0]) and not same(other["gA"][7], out["gA"][7])


# ============================================================================================ dropout
DROP_CASES = [2, 4]
KEYS = [(0x1234567, 64 * 3 + 1), (0x9E3779B97F4A7C15, 64 * 1000 + 63)]   # (seed, stream = step * 64 + layer)


def window_bank(D, w):
    """bankA with A[j][k] = (k == 16 w + j) in every slot and layer: stage A on ones reads out the mask of columns [16 w, 16 w + 16)"""
    a = np.zeros((SLOTS, LAYERS, 16, D), np.float32)
    a[:, :, np.arange(16), 16 * w + np.arange(16)] = 1.0
    return a


@functools.lru_cache(maxsize=None)
def bank_mask(case, dt, p, seed, stream):
    """the dropout mask of the bank's stage A, read out window by window: [rows][Ttok][D] of keep (kept) or 0; the slot -1 row is NaN"""
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    c = problem(case, dt)
    ones = np.ones((ROWS, T, D), np.float32)
    m = np.full((ROWS, T, D), np.nan, np.float32)
    for w in range(D // 16):
        out = run(case, dt, c, A, over={"xn": ones, "bankA": window_bank(D, w)}, train=1, p=p, seed=seed, stream=stream)
        assert np.all(out["La"][1] == SENT)
        m[ACTIVE, :, 16 * w:16 * w + 16] = out["La"][ACTIVE]
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def model_mask(n, dt, p, seed, stream):
    """rsys_op_dropout on n ones: the finetune model's kernel is the specification of the mask"""
    bf = Bufs(64)
    try:
        src = bf.put(np.ones(n, np.float32), dt); dst = bf.put(np.full(n, SENT, np.float32), dt)
        assert bf.L.rsys_op_dropout(dt, src, dst, n, C.c_float(p), seed, stream, 0) == 0, _lib().last_error()
        return bf.get(dst, (n,), dt)
    finally:
        bf.free()


@pytest.mark.parametrize("case", DROP_CASES)
def test_dropout_mask_is_the_finetune_models(case):
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    n = ROWS * T * D
    masks = {}
    for seed, stream in KEYS:
        for dt in DTYPES:
            m = bank_mask(case, dt, 0.5, seed, stream)
            assert set(np.unique(m[ACTIVE])) == {0.0, 2.0}                                 # ones under p = 0.5: exactly 0 or 2
            spec = model_mask(n, dt, 0.5, seed, stream).reshape(ROWS, T, D)
            assert same(m[ACTIVE], spec[ACTIVE]), ("the bank's mask is not launch_dropout's", case, dt, seed)   # 1.
            masks[(dt, stream)] = m[ACTIVE]
            kept = float((m[ACTIVE] != 0).mean()); cnt = m[ACTIVE].size
            assert abs(kept - 0.5) <= 5 * math.sqrt(0.25 / cnt), kept                       # 4. at p = 0.5
        assert same(masks[(F32, stream)], masks[(BF16, stream)])                             # 2.
    assert not same(masks[(F32, KEYS[0][1])], masks[(F32, KEYS[1][1])])                      # 3.
    assert 0.4 < float((masks[(F32, KEYS[0][1])] == masks[(F32, KEYS[1][1])]).mean()) < 0.6   # two independent fair masks


def test_dropout_keep_rate_p01():
    case, p = 4, 0.1                                                                         # the larger dropout case
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    for dt in DTYPES:
        seed, stream = KEYS[0]
        m = bank_mask(case, dt, p, seed, stream)[ACTIVE]
        keep = float(storage(np.float32([ab.keep_of(p)]), dt)[0])                            # ones under p: 0 or keep in the compute type
        assert set(np.unique(m)) == {0.0, keep}
        kept = float((m != 0).mean())
        assert abs(kept - 0.9) <= 5 * math.sqrt(p * (1 - p) / m.size), kept
        spec = model_mask(ROWS * T * D, dt, p, seed, stream).reshape(ROWS, T, D)[ACTIVE]
        assert same(m, spec)


@pytest.mark.parametrize("case", DROP_CASES)
@pytest.mark.parametrize("dt", DTYPES)
def test_dropout_backward_uses_the_same_mask(case, dt):
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    c = problem(case, dt)
    ones = np.ones((ROWS, T, D), np.float32)
    for seed, stream in KEYS:
        m = bank_mask(case, dt, 0.5, seed, stream)                                          # keep * mask = 0 or 2
        # dx: dLa of ones and the window bank give u = 1 on the window's columns and 0 elsewhere: dxn = 0 + keep * mask there
        got = np.zeros((ROWS, T, D), np.float32)
        for w in range(D // 16):
            out = run(case, dt, c, DX, over={"dLa": np.ones((ROWS, T, 16)), "bankA": window_bank(D, w), "dxn": np.zeros((ROWS, T, D))}, p=0.5,
                      seed=seed, stream=stream)
            cols = np.r_[16 * w:16 * w + 16]
            rest = np.setdiff1d(np.arange(D), cols)
            assert np.all(out["dxn"][..., rest] == 0) and np.all(out["dxn"][1] == 0)
            got[..., cols] = out["dxn"][..., cols]
        assert same(got[ACTIVE], m[ACTIVE]), "dx draws another mask than stage A"
        # dA: dLa[t][j] = (j == t % 16), xn = ones: partA[r][j][d] = keep * (the mask's sum over the row's tokens t = j mod 16): small integers
        # times 2, exact in fp32
        dla_hot = (np.arange(T)[:, None] % 16 == np.arange(16)[None, :]).astype(np.float32)
        out = run(case, dt, c, DA, over={"dLa": np.broadcast_to(dla_hot, (ROWS, T, 16)), "xn": ones}, p=0.5, seed=seed, stream=stream)
        want = np.einsum("tj,rtd->rjd", dla_hot.astype(np.float64), m[ACTIVE].astype(np.float64))
        assert np.array_equal(out["partA"][ACTIVE].astype(np.float64), want), "dA draws another mask than stage A"
        assert np.all(out["partA"][1] == SENT)


@pytest.mark.parametrize("case", DROP_CASES)
@pytest.mark.parametrize("dt", DTYPES)
def test_dropout_random_data_p025(case, dt):
    """a_train, dA and dx on random data at p = 0.25 against the reference under the mask read out of stage A (non-zero = kept)"""
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    p = 0.25
    seed, stream = KEYS[1]
    c, o0 = problem(case, dt), reference(case, dt)
    act = ACTIVE
    mask = (np.nan_to_num(bank_mask(case, dt, p, seed, stream)) != 0).astype(np.float64)
    assert abs(mask[act].mean() - 0.75) <= 5 * math.sqrt(p * (1 - p) / mask[act].size)
    xn, dxn, bankA = f64(c, "xn", "dxn", "bankA")
    xd = ab.dropped(xn, mask, p, dt)
    keep = ab.keep_of(p)
    what = f"case {case} p 0.25"
    # stage A of a training pass: the same sums over drop(xn), which is rounded to the compute type like an input
    la, la_mag = ab.stage_a(xd, bankA, ROW_SLOT, LAYER)
    out = run(case, dt, c, A, train=1, p=p, seed=seed, stream=stream)
    untouched(case, out, A)
    check("a_train", dt, out["La"][act], la[act], (c_stage_a(D, dt) + 1) * U * la_mag[act], True, what)
    # dA partials over drop(xn)
    pa, pa_mag = ab.da(o0["dLa"], xd, ROW_SLOT)
    out = run(case, dt, c, DA, over={"dLa": o0["dLa"]}, p=p, seed=seed, stream=stream)
    untouched(case, out, DA)
    check("da.drop", dt, out["partA"][act], pa[act], (c_tokens(T, dt) + 1) * U * pa_mag[act], False, what)
    # dx: 16 fmas; rounded to the compute type where the reference rounds too (a sum within its bound of a rounding boundary may land
    # one bf16 ulp away: + ulp(u) under the scale); x keep; + old
    ref = ab.dx_finish(o0["u"], dxn, mask, p, dt)
    first = (16 + 1) * U * o0["u_mag"] + (bf16_ulp(o0["u"]) if dt == BF16 else 0.0)
    bound = keep * mask * first + (2 + 1) * U * (np.abs(dxn) + keep * mask * np.abs(o0["u"])) + 1e-300
    out = run(case, dt, c, DX, over={"dLa": o0["dLa"]}, p=p, seed=seed, stream=stream)
    untouched(case, out, DX)
    check("dx.drop", dt, out["dxn"][act], ref[act], bound[act], True, what)
    if dt != BF16:
        return
    # the extra rounding point, in bf16 on a zero dxn: dx = bf16(fl32(bf16(u) keep)), NOT bf16(fl32(u keep)).  Wherever the two differ (and u is
    # not within its fp32 bound of a bf16 rounding boundary, where the kernel's sum may round the other way) the kernel gives the first.
    out = run(case, dt, c, DX, over={"dLa": o0["dLa"], "dxn": np.zeros((ROWS, T, D))}, p=p, seed=seed, stream=stream)
    u = o0["u"][act]; k32 = np.float32(keep)
    r1 = bf16_round(bf16_round(u.astype(np.float32)) * k32)
    r0 = bf16_round((u * keep).astype(np.float32))
    edge = np.abs(np.abs(u - bf16_round(u.astype(np.float32)).astype(np.float64)) - 0.5 * bf16_ulp(u)) <= (16 + 1) * U * o0["u_mag"][act]
    sel = (mask[act] != 0) & ~edge
    differ = sel & (r1 != r0)
    assert differ.sum() > 100, differ.sum()
    assert np.array_equal(out["dxn"][act][sel], r1[sel])
    assert np.all(out["dxn"][act][mask[act] == 0] == 0)


# ============================================================================================ optimizer
def _slot_recs():
    """(active, lr, max_norm, step) of the eight slots: 1 unclipped, 5 clipped, 6 without a clip, 2 at step 7, 3 inactive"""
    rec = np.zeros((SLOTS, 4), np.float32)
    for s in range(SLOTS):
        rec[s] = (1.0, 1e-2 * (1 + 0.25 * s), 1.0, 1)
    rec[1, 2] = 1e6; rec[5, 2] = 1.0; rec[6, 2] = 0.0; rec[2, 3] = 7; rec[4, 3] = 1000
    rec[3] = (0.0, 1e-2, 1.0, 1)
    return rec


@pytest.mark.parametrize("case", [3, 7])
@pytest.mark.parametrize("dt", DTYPES)
def test_bank_adamw(case, dt):
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    nA, nB = LAYERS * 16 * D, LAYERS * (Nq + Nk) * 8
    assert (nA, nB) == {3: (2560, 2560), 7: (4096, 3072)}[case]
    rng = np.random.default_rng(40 + case + dt)
    rec = _slot_recs()
    h = {}
    for part, n in (("A", nA), ("B", nB)):
        h["p" + part] = (0.1 * rng.standard_normal((SLOTS, n))).astype(np.float32)
        h["g" + part] = (0.05 * rng.standard_normal((SLOTS, n))).astype(np.float32)    # |g| ~ 0.05 sqrt(nA + nB) ~ 4: max_norm 1 clips
        h["m" + part] = (0.01 * rng.standard_normal((SLOTS, n))).astype(np.float32)
        h["v" + part] = (0.001 * rng.uniform(0.1, 1.0, (SLOTS, n))).astype(np.float32)
        h["s" + part] = np.full((SLOTS, n), SENT, np.float32)
    first = (rec[:, 3] == 1) & (rec[:, 0] != 0)
    for k in ("mA", "vA", "mB", "vB"):
        h[k][first] = 0.0                                                                # a first step starts from zero moments
    bf = Bufs(64)
    try:
        d = {k: bf.put(v, BF16 if (k[0] == "s" and dt == BF16) else F32) for k, v in h.items()}
        dn = bf.put(np.full(SLOTS, SENT, np.float32))
        a = ADAM
        rc = bf.L.rsys_op_adapter_bank_adamw(dt, d["pA"], d["pB"], d["gA"], d["gB"], d["mA"], d["vA"], d["mB"], d["vB"], d["sA"] if dt == BF16 else None,
                                             d["sB"] if dt == BF16 else None, nA, nB, rec.ctypes.data, C.c_float(a["b1"]), C.c_float(a["b2"]),
                                             C.c_float(a["eps"]), C.c_float(a["wd"]), dn)
        assert rc == 0, _lib().last_error()
        o = {k: bf.get(d[k], v.shape, BF16 if (k[0] == "s" and dt == BF16) else F32) for k, v in h.items()}
        norms = bf.get(dn, (SLOTS,))
    finally:
        bf.free()
    for s in range(SLOTS):
        if not rec[s, 0]:
            for k in h:
                assert same(o[k][s], h[k][s]), (s, k, "an inactive slot was written")
            assert norms[s] == 0
            continue
        j = lambda x, name: np.concatenate([x[name + "A"][s], x[name + "B"][s]])       # noqa: E731  the slot's tensors, A then B
        step, max_norm, lr = int(rec[s, 3]), float(rec[s, 2]), float(rec[s, 1])
        adam = dict(ADAM, lr=lr)
        n = nA + nB
        p_ref, m_ref, v_ref, e_p, e_m, e_v, coef, crel, ss_ref = _adamw_ref(j(h, "p"), j(h, "g"), j(h, "m"), j(h, "v"), n, step=step,
                                                                             max_norm=max_norm, grad_div=1.0, **adam)
        # the norm: all terms positive, so the longest chain bounds the relative error of the sum: ceil(nA / 1024) + ceil(nB / 1024) fmas into a
        # thread's accumulator, 6 shuffle levels, 16 LDS adds; the square root halves it and rounds once (crel above assumes <= 64)
        chain = math.ceil(nA / 1024) + math.ceil(nB / 1024) + 6 + 16
        assert chain <= 64
        nref = math.sqrt(ss_ref)
        r = abs(norms[s] - nref) / ((0.5 * chain + 1 + 1) * U * nref)
        print(f"ratio adamw.norm {'bf16' if dt == BF16 else 'fp32'} case {case} slot {s}: {r:.3f}")
        assert r <= 1.0, (s, norms[s], nref)
        assert (coef < 1.0) == (s not in (1, 6)), (s, coef)                           # which slots clip
        for name, ref, e in (("m", m_ref, e_m), ("v", v_ref, e_v), ("p", p_ref, e_p)):
            err = np.abs(j(o, name) - ref) - e
            assert err.max() <= 0, (s, name, float(err.max()), int(np.argmax(err)))
        assert not np.any(j(o, "g")), (s, "the gradient is not zeroed")
        if dt == BF16:
            assert same(j(o, "s"), bf16_round(j(o, "p"))), (s, "the bf16 copy is not the rounded new master")
        else:
            assert np.all(j(o, "s") == SENT)


# ============================================================================================ refusals
REFUSALS = [
    (dict(args=dict(Ttok=12)), "Ttok % 8"),
    (dict(args=dict(D=24, H=1, hd=24)), "D % 16"),
    (dict(args=dict(D=32, H=1, hd=16)), "H * hd"),
    (dict(args=dict(D=16, H=2, hd=8)), "hd must be"),
    (dict(args=dict(D=48, H=3, KV=2, hd=16)), "H % KV"),
    (dict(args=dict(layer=2)), "layer"),
    (dict(row_slot=[3, -1, 0, 3, 8]), "row_slot"),
    (dict(row_slot=[3, -2, 0, 3, 7]), "row_slot"),
    (dict(p=1.0), "dropout p"),
    (dict(p=-0.125), "dropout p"),
    (dict(pos="high"), "rope_pos"),
    (dict(pos="negative"), "rope_pos"),
    (dict(explicit_pos=False, rope_rows=16), "rope tables"),
]


@pytest.mark.parametrize("dt", DTYPES)
def test_refusals_leave_the_outputs_unwritten(dt):
    case = 2
    T, D, H, KV, hd, Nq, Nk, ld = dims(case)
    c = problem(case, dt)
    for kw, msg in REFUSALS:
        kw = dict(kw)
        if isinstance(kw.get("pos"), str):
            pos = np.array(c["pos"])
            pos[4, T - 1] = T + 13 if kw["pos"] == "high" else -1
            kw["pos"] = pos
        out = run(case, dt, c, ALL, train=1, expect_error=msg, **kw)
        for k in OUTPUTS:
            assert same(out[k], out["prefill"][k]), (msg, k)
