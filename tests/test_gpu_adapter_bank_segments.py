"""GPU: the adapter bank's kernels in the forms of packed finetune rows (csrc/adapter_bank.hip) through
rsys_op_adapter_bank_segments (rsys_debug.h): the token stages with the slot of the workgroup's tile (a with DROP, b, dla, dx; printed as
a_train_tiles, b_tiles, dla_tiles, dx_tiles), the partials per segment (da, db; printed as da_seg, db_seg) and the reduction over the
segment table (segs_reduce) -- the tile / segment path of each stage's one kernel -- in fp32 and bf16, on sentinel-filled outputs with
guard tails.

  case  Ttok  D   H KV hd   rows  what it covers
  1      72  160  5 1  32    3    a ragged second tile (8 tokens); two one-tile segments in a row; a row whose second tile nobody owns
  2     136  320  5 5  64    3    three tiles: a two-tile segment plus a ragged one; a segment ending in the ragged tile; unowned tiles 0 and 2
  3     200   48  3 1  16    2    segments of tiles {0, 1} and {3}, tile 2 unowned; hd 16 gives bf16 dLa its ragged K steps
  4     256  128  2 1  64    2    the whole-model shape: four one-tile segments in two rows
  5     192  256  2 1 128    2    hd 128

Layer 1 of L = 2; the tables mix slots {3, -1, 0, 7}, slot 3 always has two segments that are not neighbours in the table.

Checks: (1) every stage alone on reference intermediates and all stages in one call against the float64 restatement of
tests/_adapter_bank_seg_np.py, with tests/test_gpu_adapter_bank_ops.py's rounding-count bounds (a segment's partial counts the tokens of
the SEGMENT's range; the reduction of a slot with n segments counts n roundings); (2) bit equality with the row-slot kernels: token
stages tile by tile against the row kernel run with that tile's slot on every row (dropout 0.25 included: same element indices), the
per-segment partials against the row kernel on buffers zeroed outside the segment (also with -0.0 and with finite values in the other
operand); (3) everything a call must not write stays bit for bit; (4) accumulation in descriptor order, and a slot's gradient does not
move when descriptors of other slots are reordered; (5) a repeated call gives equal bits; (6) refusals leave the outputs unwritten.
Each comparison prints its figure (`pytest -s`)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _adapter_bank_np as ab
import _adapter_bank_seg_np as sg
from test_gpu_adapter_bank_ops import Bufs, c_dla, c_stage_a, c_tokens, check, f64, rope_tables, same
from test_gpu_row_kernels import BF16, F32, SENT, U, _lib, bf16_ulp, storage

pytestmark = pytest.mark.gpu

DTYPES = [F32, BF16]
LAYERS, LAYER, SLOTS = 2, 1, 8
CASES = {1: (72, 160, 5, 1, 32, 3), 2: (136, 320, 5, 5, 64, 3), 3: (200, 48, 3, 1, 16, 2), 4: (256, 128, 2, 1, 64, 2), 5: (192, 256, 2, 1, 128, 2)}
# (row, first column, columns, slot, task)
SEGS = {1: [(0, 0, 30, 3, 1), (1, 0, 20, -1, -1), (0, 32, 4, 0, 0), (1, 32, 3, 7, 2), (2, 0, 32, 3, 1)],
        2: [(0, 0, 50, 3, 1), (0, 64, 4, 0, 0), (1, 0, 10, -1, -1), (1, 32, 36, 7, 3), (2, 32, 20, 3, 1)],
        3: [(0, 0, 64, 3, 1), (0, 96, 4, 0, 0), (1, 0, 33, 7, 2), (1, 64, 32, -1, -1), (1, 96, 2, 3, 1)],
        4: [(0, 0, 32, 3, 1), (0, 64, 5, 0, 0), (1, 32, 31, -1, -1), (1, 96, 32, 3, 1)],
        5: [(0, 0, 40, 7, 2), (0, 64, 32, 3, 1), (1, 0, 32, 0, 0), (1, 32, 10, -1, -1), (1, 64, 1, 3, 1)]}
A, B, DLA, DB, DA, DX, RED, ALL = 1, 2, 4, 8, 16, 32, 64, 127
OUTPUTS = ("La", "qkv", "dLa", "dxn", "partA", "partB", "gA", "gB")
FP32_BUFS = ("partA", "partB", "gA", "gB")
WRITES = {"La": A, "qkv": B, "dLa": DLA, "dxn": DX, "partA": DA, "partB": DB, "gA": RED, "gB": RED}


def dims(case):
    T, D, H, KV, hd, rows = CASES[case]
    Nq, Nk = H * hd, KV * hd
    return T, D, H, KV, hd, rows, Nq, Nk, Nq + 2 * Nk


def segs_of(case):
    return np.asarray(SEGS[case], np.int32)


@functools.lru_cache(maxsize=None)
def problem(case, dt):
    T, D, H, KV, hd, rows, Nq, Nk, ld = dims(case)
    rng = np.random.default_rng(4100 + 10 * case + dt)
    c = {"xn": storage(rng.standard_normal((rows, T, D)), dt), "qkv": storage(rng.standard_normal((rows, T, ld)), dt),
         "dqkv": storage(0.5 * rng.standard_normal((rows, T, ld)), dt), "dxn": storage(rng.standard_normal((rows, T, D)), dt),
         "La_in": storage(rng.standard_normal((rows, T, 16)), dt), "dLa_in": storage(rng.standard_normal((rows, T, 16)), dt),
         "bankA": storage(0.1 * rng.standard_normal((SLOTS, LAYERS, 16, D)), dt),
         "bankB": storage(0.1 * rng.standard_normal((SLOTS, LAYERS, Nq + Nk, 8)), dt),
         "gA": rng.standard_normal((SLOTS, LAYERS, 16, D)).astype(np.float32),
         "gB": rng.standard_normal((SLOTS, LAYERS, Nq + Nk, 8)).astype(np.float32),
         "pos": rng.integers(0, T + 13, (rows, T)).astype(np.int32)}
    c["cos"], c["sin"] = rope_tables(T, hd)
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(case, dt):
    """the fp64 chain with the rounding points applied; shared by the tests, never modified"""
    c = problem(case, dt)
    T, D, H, KV, hd, rows, Nq, Nk, ld = dims(case)
    xn, qkv, dqkv, dxn, bankA, bankB, gA, gB = f64(c, "xn", "qkv", "dqkv", "dxn", "bankA", "bankB", "gA", "gB")
    return sg.chain(dt, xn, qkv, dqkv, dxn, bankA, bankB, SEGS[case], LAYER, gA, gB, H, KV, hd, c["cos"], c["sin"], c["pos"])


def run(case, dt, stages, table, segments=True, over=None, train=0, p=0.0, seed=0, stream=0, args=None, n_seg=None, expect_error=None):
    """one call on freshly uploaded buffers: `segments` -> rsys_op_adapter_bank_segments with the table [n][5], else rsys_op_adapter_bank
    with `table` = row_slot [rows].  Pure outputs start as the sentinel; returns every output buffer (guard tails checked) + the prefill"""
    T, D, H, KV, hd, rows, Nq, Nk, ld = dims(case)
    c = problem(case, dt)
    table = None if table is None else np.asarray(table, np.int32)
    nparts = rows if not segments else (len(SEGS[case]) if table is None else max(1, table.shape[0]))
    h = {k: c[k] for k in ("xn", "qkv", "dqkv", "dxn", "bankA", "bankB", "gA", "gB")}
    h["La"] = np.full((rows, T, 16), SENT, np.float32); h["dLa"] = np.full((rows, T, 16), SENT, np.float32)
    h["partA"] = np.full((nparts, 16, D), SENT, np.float32); h["partB"] = np.full((nparts, Nq + Nk, 8), SENT, np.float32)
    for k, v in (over or {}).items():
        h[k] = storage(v, F32 if k in FP32_BUFS else dt)
    bf = Bufs(32 * max(ld, D))
    try:
        d = {k: bf.put(v, F32 if k in FP32_BUFS else dt) for k, v in h.items()}
        dtab = bf.put(table if table.size else np.zeros(5, np.int32)) if table is not None else None
        dcos, dsin, dpos = bf.put(c["cos"]), bf.put(c["sin"]), bf.put(c["pos"])
        a = dict(rows=rows, Ttok=T, D=D, H=H, KV=KV, hd=hd, L=LAYERS, layer=LAYER)
        a.update(args or {})
        head = (dt, stages, train, a["rows"], a["Ttok"], a["D"], a["H"], a["KV"], a["hd"], a["L"], a["layer"], C.c_float(p), seed, stream)
        tail = (d["bankA"], d["bankB"], d["xn"], d["La"], d["qkv"], d["dqkv"], d["dLa"], d["dxn"], d["partA"], d["partB"], d["gA"], d["gB"], dcos, dsin,
                dpos, c["cos"].shape[0])
        if segments:
            rc = bf.L.rsys_op_adapter_bank_segments(*head, dtab, (0 if table is None else table.shape[0]) if n_seg is None else n_seg, *tail)
        else:
            rc = bf.L.rsys_op_adapter_bank(*head, dtab, *tail)
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


def untouched(case, out, stages, table=None):
    """everything a segments call must leave bit for bit: what no selected stage writes; in the token buffers the tiles nobody owns, the
    tiles of -1 segments and the k columns; the partials of -1 segments; in the gradients layer 0 and the slots without a segment"""
    T, D, H, KV, hd, rows, Nq, Nk, ld = dims(case)
    table = SEGS[case] if table is None else table
    h = out["prefill"]
    dead = sg.token_slot(table, rows, T) < 0
    named = set(s for s in sg.seg_slots(table) if s >= 0)
    assert dead.any() and len(named) < SLOTS
    for k in OUTPUTS:
        if not stages & WRITES[k]:
            assert same(out[k], h[k]), (k, "written by a stage that was not selected")
        elif k in ("gA", "gB"):
            assert same(out[k][:, 0], h[k][:, 0]), (k, "layer 0")
            rest = [s for s in range(SLOTS) if s not in named]
            assert same(out[k][rest], h[k][rest]), (k, "slots without a segment")
        elif k in ("partA", "partB"):
            off = [i for i, s in enumerate(sg.seg_slots(table)) if s < 0]
            assert same(out[k][off], h[k][off]), (k, "the partial of a -1 segment")
        else:
            assert same(out[k][dead], h[k][dead]), (k, "an unowned tile or a -1 segment")
    if stages & B:
        assert same(out["qkv"][..., Nq:Nq + Nk], h["qkv"][..., Nq:Nq + Nk]), "k columns"


def b_bound(case, mag):
    """stage B: 11 roundings on the q columns, 9 on the v columns (test_gpu_adapter_bank_ops.py)"""
    T, D, H, KV, hd, rows, Nq, Nk, ld = dims(case)
    cnt = np.zeros(ld); cnt[:Nq] = 11 + 1; cnt[Nq + Nk:] = 9 + 1
    return cnt * U * mag


def c_seg_tokens(case, dt):
    """per segment: the roundings of one wave's contraction over the segment's token range, [n_seg][1][1]"""
    T = CASES[case][0]
    return np.asarray([c_tokens(ke - kb, dt) for kb, ke in (sg.token_range(s, T) for s in SEGS[case])], np.float64)[:, None, None]


def c_reduce(case):
    """per slot: n - 1 additions of n segments (the first is added to zero exactly) + 1 (+ g), [SLOTS][1][1]; at least the row test's 2"""
    n = np.bincount([s for s in sg.seg_slots(SEGS[case]) if s >= 0], minlength=SLOTS)
    return np.maximum(n, 2).astype(np.float64)[:, None, None]


def live(case):
    T, D, H, KV, hd, rows, Nq, Nk, ld = dims(case)
    return sg.token_slot(SEGS[case], rows, T) >= 0


def live_segs(case):
    return [i for i, s in enumerate(sg.seg_slots(SEGS[case])) if s >= 0]


def named(case):
    return sorted(set(s for s in sg.seg_slots(SEGS[case]) if s >= 0))


# ============================================================================================ (1) bounds: every stage alone
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
def test_stages_alone(case, dt):
    T, D, H, KV, hd, rows, Nq, Nk, ld = dims(case)
    c, o = problem(case, dt), reference(case, dt)
    tab, act, ls, sl = SEGS[case], live(case), live_segs(case), named(case)
    qv = np.r_[0:Nq, Nq + Nk:ld]
    what = f"segments case {case}"
    out = run(case, dt, A, tab, train=1, p=0.0, seed=11, stream=70)
    untouched(case, out, A)
    check("a_train_tiles", dt, out["La"][act], o["La64"][act], (c_stage_a(D, dt) + 1) * U * o["La_mag"][act], True, what)
    out = run(case, dt, B, tab, over={"La": o["La"]})
    untouched(case, out, B)
    check("b_tiles", dt, out["qkv"][act][..., qv], o["qkv"][act][..., qv], b_bound(case, o["qkv_mag"])[act][..., qv], True, what)
    out = run(case, dt, DLA, tab)
    untouched(case, out, DLA)
    check("dla_tiles", dt, out["dLa"][act], o["dLa64"][act], (c_dla(Nq, Nk, dt) + 1) * U * o["dLa_mag"][act], True, what)
    cs = c_seg_tokens(case, dt)
    out = run(case, dt, DB, tab, over={"La": o["La"]})
    untouched(case, out, DB)
    check("db_seg", dt, out["partB"][ls], o["partB"][ls], ((cs + 1) * U * o["partB_mag"])[ls], False, what)
    out = run(case, dt, DA, tab, over={"dLa": o["dLa"]})
    untouched(case, out, DA)
    check("da_seg", dt, out["partA"][ls], o["partA"][ls], ((cs + 1) * U * o["partA_mag"])[ls], False, what)
    out = run(case, dt, DX, tab, over={"dLa": o["dLa"]})
    untouched(case, out, DX)
    check("dx_tiles", dt, out["dxn"][act], o["dxn"][act], ((17 + 1) * U * (o["u_mag"] + np.abs(c["dxn"])))[act], True, what)
    # the reduction on the reference partials (as fp32), added to the prefilled gradients: a slot's segments in descriptor order, bit for bit
    pa, pb = o["partA"].astype(np.float32), o["partB"].astype(np.float32)
    out = run(case, dt, RED, tab, over={"partA": pa, "partB": pb})
    untouched(case, out, RED)
    assert same(out["gA"], ab.reduce32(pa, sg.seg_slots(tab), c["gA"], LAYER, 1.0)) and same(out["gB"], ab.reduce32(pb, sg.seg_slots(tab), c["gB"], LAYER, 2.0))
    for name, part, alpha in (("gA", pa, 1.0), ("gB", pb, 2.0)):
        ref, mag = ab.reduce(part.astype(np.float64), sg.seg_slots(tab), np.asarray(c[name], np.float64), LAYER, alpha)
        check("segs_reduce", dt, out[name][sl, LAYER], ref[sl, LAYER], ((c_reduce(case) + 1) * U * mag[:, LAYER])[sl], False, f"{what} {name}")
        assert not same(out[name][sl, LAYER], c[name][sl, LAYER])


# ============================================================================================ (1, 3, 5) all stages in one call
def allowances(case, dt, c, o):
    """test_gpu_adapter_bank_ops.py's allowances over a segment table: every stage's own bound plus the reference's sensitivity to the stored
    inputs that stage read (all maps are linear in the intermediate)"""
    T, D, H, KV, hd, rows, Nq, Nk, ld = dims(case)
    tab = SEGS[case]
    ts = sg.token_slot(tab, rows, T).ravel()
    back = lambda x: x.reshape(rows, T, x.shape[-1])
    ulp = (lambda x: bf16_ulp(x)) if dt == BF16 else (lambda x: 0.0)
    bankA, bankB, dqkv = f64(c, "bankA", "bankB", "dqkv")
    La_err = (c_stage_a(D, dt) + 1) * U * o["La_mag"] + ulp(o["La64"])
    dLa_err = (c_dla(Nq, Nk, dt) + 1) * U * o["dLa_mag"] + ulp(o["dLa64"])
    sq, sv = ab.stage_b_update(sg.tok(La_err), bankB, ts, LAYER, H, KV, hd, c["cos"], c["sin"], c["pos"].reshape(-1, 1), absolute=True)
    al = {"qkv": b_bound(case, o["qkv_mag"])}
    al["qkv"][..., :Nq] += back(sq); al["qkv"][..., Nq + Nk:] += back(sv)
    al["dxn"] = (17 + 1) * U * (o["u_mag"] + np.abs(c["dxn"])) + back(ab.dx_sum(sg.tok(dLa_err), bankA, ts, LAYER)[1])
    cs = c_seg_tokens(case, dt)
    partA_err = (cs + 1) * U * o["partA_mag"] + sg.da(dLa_err, o["xd"], tab)[1]
    partB_err = (cs + 1) * U * o["partB_mag"] + sg.db(dqkv, La_err, tab, H, KV, hd)[1]
    zA, zB = np.zeros_like(o["gA"]), np.zeros_like(o["gB"])
    cr = c_reduce(case)[:, None]
    al["gA"] = (cr + 1) * U * o["gA_mag"] + ab.reduce(partA_err, sg.seg_slots(tab), zA, LAYER, 1.0)[0]
    al["gB"] = (cr + 1) * U * o["gB_mag"] + ab.reduce(partB_err, sg.seg_slots(tab), zB, LAYER, 2.0)[0]
    return al


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
def test_one_call_and_repeat(case, dt):
    T, D, H, KV, hd, rows, Nq, Nk, ld = dims(case)
    c, o = problem(case, dt), reference(case, dt)
    act, sl = live(case), named(case)
    qv = np.r_[0:Nq, Nq + Nk:ld]
    al = allowances(case, dt, c, o)
    what = f"segments one call, case {case}"
    out = run(case, dt, ALL, SEGS[case], train=1)
    untouched(case, out, ALL)
    check("all/qkv", dt, out["qkv"][act][..., qv], o["qkv"][act][..., qv], al["qkv"][act][..., qv], True, what)
    check("all/dxn", dt, out["dxn"][act], o["dxn"][act], al["dxn"][act], True, what)
    check("all/gA", dt, out["gA"][sl, LAYER], o["gA"][sl, LAYER], al["gA"][sl, LAYER], False, what)
    check("all/gB", dt, out["gB"][sl, LAYER], o["gB"][sl, LAYER], al["gB"][sl, LAYER], False, what)
    again = run(case, dt, ALL, SEGS[case], train=1)
    for k in OUTPUTS:
        assert same(out[k], again[k]), (k, "a repeated call differs")


# ============================================================================================ (2) equality with the row-slot kernels
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
def test_token_stages_equal_the_row_slot_kernels_tile_by_tile(case, dt):
    T, D, H, KV, hd, rows, Nq, Nk, ld = dims(case)
    c = problem(case, dt)
    ts = sg.token_slot(SEGS[case], rows, T)
    runs = [("a_train p 0", A, "La", dict(train=1, p=0.0, seed=5, stream=65)), ("a_train p 0.25", A, "La", dict(train=1, p=0.25, seed=5, stream=65)),
            ("b", B, "qkv", dict(over={"La": c["La_in"]})), ("dla", DLA, "dLa", {}),
            ("dx p 0", DX, "dxn", dict(over={"dLa": c["dLa_in"]})), ("dx p 0.25", DX, "dxn", dict(over={"dLa": c["dLa_in"]}, p=0.25, seed=5, stream=65))]
    for name, stage, key, kw in runs:
        got = run(case, dt, stage, SEGS[case], **kw)
        want = got["prefill"][key].astype(np.float32).copy()
        for s in named(case):
            ref = run(case, dt, stage, [s] * rows, segments=False, **kw)[key]
            want[ts == s] = ref[ts == s]
        diff = int((got[key].view(np.uint32) != np.ascontiguousarray(want, np.float32).view(np.uint32)).sum())
        print(f"tiles vs rows, case {case} {'bf16' if dt == BF16 else 'fp32'} {name}: {diff} of {want.size} values differ")
        assert diff == 0, name
        assert not same(got[key][ts >= 0], got["prefill"][key][ts >= 0]), name
    a0 = run(case, dt, A, SEGS[case], train=1, p=0.0, seed=5, stream=65)["La"]
    a1 = run(case, dt, A, SEGS[case], train=1, p=0.25, seed=5, stream=65)["La"]
    assert not same(a0, a1), "the dropout mask changed nothing"


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
def test_segment_partials_equal_the_row_kernels_on_zeroed_rows(case, dt):
    """partial i of the segment form == the row kernel's partial of the segment's row when the contraction's gradient operand is zero
    outside the segment's range: +0.0 in both operands, then -0.0 in the gradient operand with the other operand left finite"""
    T, D, H, KV, hd, rows, Nq, Nk, ld = dims(case)
    c = problem(case, dt)
    tab = SEGS[case]
    for p in (0.0, 0.25):
        kw = dict(train=1, p=p, seed=9, stream=65)
        got = run(case, dt, DA | DB, tab, over={"dLa": c["dLa_in"], "La": c["La_in"]}, **kw)
        for i in live_segs(case):
            r, slot = tab[i][0], tab[i][3]
            kb, ke = sg.token_range(tab[i], T)
            rs = [-1] * rows; rs[r] = slot
            for fill, both in ((0.0, True), (-0.0, False)):
                z = {}
                for k in ("dLa_in", "dqkv") + (("xn", "La_in") if both else ()):
                    z[k] = np.full(c[k].shape, fill, np.float32); z[k][r, kb:ke] = c[k][r, kb:ke]
                over = {"dLa": z["dLa_in"], "dqkv": z["dqkv"], "La": z.get("La_in", c["La_in"]), "xn": z.get("xn", c["xn"])}
                ref = run(case, dt, DA | DB, rs, segments=False, over=over, **kw)
                for key in ("partA", "partB"):
                    diff = int((got[key][i].view(np.uint32) != ref[key][r].view(np.uint32)).sum())
                    print(f"segment vs row partial, case {case} {'bf16' if dt == BF16 else 'fp32'} p {p} segment {i} {key} fill {fill!r} "
                          f"{'both operands' if both else 'gradient operand only'}: {diff} of {ref[key][r].size} values differ")
                    assert diff == 0, (key, i, fill)
        assert not same(got["partA"][live_segs(case)], got["prefill"]["partA"][live_segs(case)])


# ============================================================================================ (4) accumulation and descriptor order
@pytest.mark.parametrize("case", [1, 3])
@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
def test_reordering_descriptors_of_other_slots_keeps_every_slot(case, dt):
    tab = list(SEGS[case])
    base = run(case, dt, ALL, tab, train=1)
    # stable by slot: different slots change places, a slot's own segments keep their order
    order = sorted(range(len(tab)), key=lambda i: -tab[i][3])
    assert order != list(range(len(tab)))
    moved = run(case, dt, ALL, [tab[i] for i in order], train=1)
    for k in ("La", "qkv", "dLa", "dxn", "gA", "gB"):
        assert same(base[k], moved[k]), k
    for k in ("partA", "partB"):
        assert same(base[k][order], moved[k]), k
    # the same slot's segments exchanged: the sum's order changes (reported, not required to differ)
    i, j = [n for n, s in enumerate(tab) if s[3] == 3]
    swap = list(tab); swap[i], swap[j] = swap[j], swap[i]
    sw = run(case, dt, ALL, swap, train=1)
    print(f"slot 3's two segments exchanged, case {case}: gA equal {same(sw['gA'], base['gA'])}, gB equal {same(sw['gB'], base['gB'])} "
          "(two terms: a + b == b + a)")


# ============================================================================================ (6) refusals
@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
def test_refusals_leave_the_outputs_unwritten(dt):
    case = 1
    tab = SEGS[case]

    def refused(err, table=tab, stages=ALL, **kw):
        out = run(case, dt, stages, table, expect_error=err, **kw)
        for k in OUTPUTS:
            assert same(out[k], out["prefill"][k]), (err, k)

    def with_seg(i, seg):
        t = list(tab); t[i] = seg
        return t

    refused("multiple of 32", with_seg(2, (0, 16, 4, 0, 0)))
    refused("multiple of 32", with_seg(2, (0, -32, 4, 0, 0)))
    refused("inside its row", with_seg(2, (0, 32, 5, 0, 0)))          # 36 columns per row
    refused("inside its row", with_seg(2, (0, 32, 0, 0, 0)))
    refused("inside its row", with_seg(2, (0, 64, 1, 0, 0)))
    refused("outside the resident batch", with_seg(2, (3, 32, 4, 0, 0)))
    refused("share a 64-token tile", with_seg(2, (0, 0, 4, 0, 0)))
    refused("share a 64-token tile", with_seg(1, (0, 32, 2, -1, -1)))   # a base-model segment owns its tile too
    refused("segment slots", with_seg(2, (0, 32, 4, 8, 0)))
    refused("segment tasks", with_seg(2, (0, 32, 4, 0, 4)))
    refused("or neither", with_seg(2, (0, 32, 4, 0, -1)))
    refused("or neither", with_seg(1, (1, 0, 20, -1, 2)))
    refused("named by two slots", with_seg(2, (0, 32, 4, 0, 1)))
    refused("n_seg must be", n_seg=0)
    refused("n_seg must be", n_seg=-1)
    refused("n_seg must be", tab + [(2, 32, 2, 5, 3), (2, 32, 2, 5, 3)])   # 7 > rows * ceil(36 / 32) = 6
    refused("is null", None, n_seg=5)
    refused("stages is a mask", stages=0)
    refused("Ttok % 8", args=dict(Ttok=68))
    refused("D must be H * hd", args=dict(H=4))
    refused("layer outside", args=dict(layer=LAYERS))
    refused("dropout p", p=1.0)
