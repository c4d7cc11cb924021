"""GPU: the kernels that decide WHICH rows the products run on, one launch at a time through their C-ABI hooks (rsys_debug.h): position
selection in both forms, the token union, the selected-first order, the row movers around them, the column-sum / cast passes of the table
gradient and the batched bf16 transpose.  Each is compared with the plain NumPy restatement of tests/_index_np.py (pinned on the CPU by
tests/test_index_np.py).

Integer outputs and moved rows are asserted EQUAL; sums are made exact by their inputs (small integers times 2^-3, weights from {0, 0.25,
0.5, 1, 2}) and asserted equal too.  The only tolerances are the three random-float column-sum cases, whose bounds are written next to the
assertion.  Every output is filled with a sentinel before the call, every buffer has a guard tail, and the shapes are the smallest that take
each branch of the launch arithmetic (named in the comment of each case)."""
import ctypes as C

import numpy as np
import pytest

import _index_np as ix

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT = -7.5           # float sentinel: exact in fp32 and bf16
SENT_H = 0xC0F0       # its bf16 bits
SENT_I = -777         # integer sentinel
GUARD = 64            # guard elements after every buffer
F32, BF16 = 0, 1
DTYPES = [F32, BF16]
ERR_ARG = -1
_GUARDS = {np.dtype(np.int32): -12345, np.dtype(np.uint32): 0xDEADBEEF, np.dtype(np.float32): SENT, np.dtype(np.uint16): SENT_H}


def _lib():
    from recommendersystem_amd import _lib
    return _lib


class Dev:
    """device buffers of one test (the pattern of test_gpu_row_kernels.py, typed): put() uploads with a guard tail, get() reads back and
    checks the guard; free() runs from the fixture, so a failing assertion or hook still frees them"""

    def __init__(self):
        self.L = _lib().lib()
        self.bufs = []

    def put(self, arr, dtype):
        dtype = np.dtype(dtype)
        h = np.concatenate([np.asarray(arr).ravel().astype(dtype), np.full(GUARD, _GUARDS[dtype], dtype)])
        p = C.c_void_p()
        assert self.L.rsys_dev_alloc(C.byref(p), h.nbytes) == 0, _lib().last_error()
        self.bufs.append(p)
        assert self.L.rsys_dev_h2d(p, h.ctypes.data, h.nbytes) == 0
        return p

    def get(self, p, shape, dtype):
        dtype = np.dtype(dtype)
        n = int(np.prod(shape))
        h = np.empty(n + GUARD, dtype)
        assert self.L.rsys_dev_d2h(h.ctypes.data, p, h.nbytes) == 0
        assert np.all(h[n:] == np.array(_GUARDS[dtype], dtype)), "write past the end of the buffer"
        return h[:n].reshape(shape)

    # T-typed float buffers: fp32, or bf16 (uploaded rounded, read back widened)
    def put_t(self, arr, dt):
        return self.put(ix.bf16_bits(arr), np.uint16) if dt == BF16 else self.put(arr, np.float32)

    def get_t(self, p, shape, dt):
        if dt == BF16:
            return (self.get(p, shape, np.uint16).astype(np.uint32) << 16).view(np.float32)
        return self.get(p, shape, np.float32)

    def free(self):
        for p in self.bufs:
            self.L.rsys_dev_free(p)
        self.bufs = []


@pytest.fixture
def dev():
    d = Dev()
    yield d
    d.free()


def _ok(rc):
    assert rc == 0, _lib().last_error()


def _off(p, nbytes):
    return C.c_void_p(p.value + nbytes)


# ============================================================================================ position selection, both forms
W_VALUES = np.array([0.25, 0.5, 1.0, 2.0], np.float32)   # sums of up to 2^16 of them are exact in fp32 in any order


def _patterns(N, rng):
    """weight patterns of one N: all zero, all positive, positives only at the very end, positives only at multiples of 64, a mix"""
    val = W_VALUES[rng.integers(0, 4, N)]
    zero = np.zeros(N, np.float32)
    last = zero.copy(); lo = N - max(1, N // 40); last[lo:] = val[lo:]        # inside the last of 32 chunks (the last position for N < 40)
    m64 = zero.copy(); m64[::64] = val[::64]
    mix = np.where(rng.random(N) < 0.3, val, 0).astype(np.float32)
    return [zero, val, last, m64, mix]


def _topks(N, pats):
    """1, N, and per pattern a cut below its number of positives (overflow) and one above it"""
    ks = {1, N}
    for w in pats:
        p = int((w > 0).sum())
        if p >= 2:
            ks.add(p // 2)
        if p < N:
            ks.add(min(N, p + max(1, (N - p) // 3)))
    return sorted(k for k in ks if 1 <= k <= N)


def _run_select(dev, form, ws, N, topk):
    nt = len(ws)
    dw = dev.put(np.stack(ws), np.float32)
    didx = dev.put(np.full(nt * topk, SENT_I), np.int32); dst = dev.put(np.full(nt * 2, SENT), np.float32); dnp = dev.put(np.full(nt, SENT_I), np.int32)
    _ok(dev.L.rsys_op_select_positions(form, nt, dw, N, topk, didx, dst, dnp))
    # (the guard tail behind idx [ntask][topk] checks that slot topk and later are not written)
    return dev.get(didx, (nt, topk), np.int32), dev.get(dst, (nt, 2), np.float32), dev.get(dnp, (nt,), np.int32)


# N < 32: the chunked form has empty chunks; N > 1024: the one-workgroup form walks ceil(N / 1024) > 1 positions per thread (1025 and 1500
# leave threads idle: 513 resp. 750 of 1024 have work); 4096 / 4100: the model's threshold, exact and ragged chunks; 20000: chunks of 625
# positions = three 256-position stripes, the last ragged; 65536: 2048 per chunk, eight full stripes, 64 positions per thread
@pytest.mark.parametrize("N", [1, 20, 1000, 1024, 1025, 1500, 4096, 4100, 20000, 65536])
def test_select_positions_both_forms(dev, N):
    rng = np.random.default_rng(N)
    pats = _patterns(N, rng)
    for topk in _topks(N, pats):
        for ws in (pats[:4], pats[4:], [pats[4], pats[1], pats[3], pats[2]]):      # 4 tasks, 1 task, 4 tasks in another order
            want = [ix.select(w, topk) for w in ws]
            got = [_run_select(dev, form, ws, N, topk) for form in (0, 1)]
            for form, (idx, stats, npos) in enumerate(got):
                for t, (ridx, rnpos, rstats) in enumerate(want):
                    assert np.array_equal(idx[t], ridx), (form, topk, t)
                    assert npos[t] == rnpos, (form, topk, t, npos[t], rnpos)
                    assert stats[t, 0] == rstats[0] and stats[t, 1] == rstats[1], (form, topk, t, stats[t], rstats)
            assert np.array_equal(got[0][0], got[1][0]), topk
        dev.free()


def test_select_positions_argument_checks(dev):
    dw = dev.put(np.zeros(16), np.float32); di = dev.put(np.zeros(64), np.int32); ds = dev.put(np.zeros(8), np.float32)
    for form, nt, N, topk in [(2, 1, 16, 4), (0, 5, 3, 1), (0, 1, 16, 17), (1, 1, 16, 0), (1, 0, 16, 4)]:
        assert dev.L.rsys_op_select_positions(form, nt, dw, N, topk, di, ds, di) == ERR_ARG


# ============================================================================================ token union
NT_MAX = 1 << 19     # launch_token_union's documented maximum: a 64 KB bitmap in dynamic LDS beside 64 bytes of static LDS


def _union_lists(NT, cap, rng):
    """four tasks over NT tokens: random positions with the extremes, an empty task, duplicates of task 0 (equal parity), an odd task.
    Entries behind npos hold valid positions that no live entry names, so reading them would show."""
    half = NT // 2
    live_pool = rng.permutation(half - 2)[: 3 * cap] + 1 if half > 2 else np.zeros(0, np.int64)      # positions 1 .. half - 2
    dead = half - 1 if half > 1 else 0                                          # even tasks' dead entries: token NT - 2, named by nobody
    n0 = min(cap - 2, live_pool.size // 3)
    t0 = np.concatenate([[0], live_pool[:n0]])                                     # token 0 included
    t1 = np.zeros(0, np.int64)
    t2 = np.concatenate([t0[: len(t0) // 2], live_pool[n0: n0 + len(t0) // 3]])    # half of task 0 again, plus new ones
    t3 = np.concatenate([[half - 1], live_pool[2 * n0: 2 * n0 + n0 // 2]]) if half >= 1 else t1      # token NT - 1 included (NT even)
    lists, npos = [], []
    for ti, t in enumerate((t0, t1, t2, t3)):
        full = np.full(cap, 0 if ti & 1 else dead, np.int64)          # (the odd tasks' dead entries: position 0 -> token 1, named by nobody)
        full[: len(t)] = t
        lists.append(full); npos.append(len(t))
    return lists, npos


def _run_union(dev, lists, npos, NT, null_mask=0):
    nt, cap = len(lists), len(lists[0])
    nw = (NT + 31) // 32
    didx = dev.put(np.stack(lists), np.int32); dnp = dev.put(npos, np.int32)
    dbits = dev.put(np.full(nw, 0xA5A5A5A5), np.uint32); dpre = dev.put(np.full(nw, SENT_I), np.int32); dn = dev.put([SENT_I], np.int32)
    rc = dev.L.rsys_op_token_union(nt, didx, cap, dnp, null_mask, NT, dbits, dpre, dn)
    return rc, dbits, dpre, dn, nw


# words per thread of the one workgroup = ceil(ceil(NT / 32) / 1024): 64, 4104 (129 words: idle threads, a partial last word) and 32768
# (1024 words) give 1; 32832 (1026 words) gives 2 with 513 busy threads; 2^19 (16384 words) gives 16
@pytest.mark.parametrize("NT", [64, 4104, 32768, 32832, NT_MAX])
def test_token_union(dev, NT):
    rng = np.random.default_rng(NT)
    cap = min(6000, NT // 2)
    lists, npos = _union_lists(NT, cap, rng)
    for null_mask, nt in [(0, 4), (4, 4), (8, 4), (0, 1), (0, 2)]:
        ls = [None if (null_mask >> t) & 1 else l for t, l in enumerate(lists[:nt])]
        toks, bits, pre, nsel = ix.token_union(ls, npos[:nt], NT)
        rc, dbits, dpre, dn, nw = _run_union(dev, lists[:nt], npos[:nt], NT, null_mask)
        _ok(rc)
        assert np.array_equal(dev.get(dbits, (nw,), np.uint32), bits), (null_mask, nt)
        assert np.array_equal(dev.get(dpre, (nw,), np.int32), pre), (null_mask, nt)
        assert dev.get(dn, (1,), np.int32)[0] == nsel == toks.size
        dev.free()
    # every task empty: an all-zero bitmap
    rc, dbits, dpre, dn, nw = _run_union(dev, lists, [0, 0, 0, 0], NT)
    _ok(rc)
    assert not dev.get(dbits, (nw,), np.uint32).any() and not dev.get(dpre, (nw,), np.int32).any() and dev.get(dn, (1,), np.int32)[0] == 0


def test_token_union_argument_checks(dev):
    lists = [np.array([0, 31, 5], np.int64), np.array([0, 31, 5], np.int64)]
    assert _run_union(dev, lists, [3, 3], 64)[0] == 0
    assert _run_union(dev, lists, [3, 3], 63)[0] == ERR_ARG              # position 31: token 2 * 31 + 1 = 63 is outside [0, 63)
    assert _run_union(dev, lists, [1, 1], 63)[0] == 0                    # ... unless that entry is not live
    assert _run_union(dev, lists, [4, 0], 64)[0] == ERR_ARG              # npos > cap
    assert _run_union(dev, lists, [3, 3], NT_MAX + 1)[0] == ERR_ARG      # the launcher's bound
    lists = [np.array([-1], np.int64)]
    assert _run_union(dev, lists, [1], 64)[0] == ERR_ARG


# ============================================================================================ selected-first order
SF_KEYS = ("slot", "sel", "perm", "uid_p", "tm_p", "pos_p", "slot_p", "sel_p", "q_active")


def _bitmap_from_union(dev, toks, NT):
    """the bitmap of a token set through the union hook (even tokens from task 0, odd ones from task 1), checked against the reference"""
    ev, od = toks[toks % 2 == 0] // 2, toks[toks % 2 == 1] // 2
    cap = max(1, ev.size, od.size)
    lists = [np.zeros(cap, np.int64), np.zeros(cap, np.int64)]
    lists[0][: ev.size] = ev[::-1]; lists[1][: od.size] = od          # (the lists need not be sorted)
    rc, dbits, dpre, dn, nw = _run_union(dev, lists, [ev.size, od.size], NT)
    _ok(rc)
    rt, bits, pre, nsel = ix.token_union(lists, [ev.size, od.size], NT)
    assert np.array_equal(rt, toks) and np.array_equal(dev.get(dbits, (nw,), np.uint32), bits) and np.array_equal(dev.get(dpre, (nw,), np.int32), pre)
    return dbits, dpre


def _run_selected_first(dev, toks, B, T, uid, tm, rope_pos):
    n, nsel = B * T, toks.size
    dbits, dpre = _bitmap_from_union(dev, toks, n)
    sel_cap = nsel + 5
    sizes = dict(slot=n, sel=sel_cap, perm=n, uid_p=n, tm_p=n, pos_p=n, slot_p=n, sel_p=sel_cap, q_active=B)
    out = {k: dev.put(np.full(sizes[k], SENT_I), np.int32) for k in SF_KEYS}
    duid = dev.put(uid, np.int32); dtm = dev.put(tm, np.int32); dpos = dev.put(rope_pos, np.int32) if rope_pos is not None else None
    _ok(dev.L.rsys_op_selected_first(dbits, dpre, B, T, duid, dtm, dpos, out["slot"], out["sel"], sel_cap, out["perm"], out["uid_p"], out["tm_p"],
                                     out["pos_p"], out["slot_p"], out["sel_p"], out["q_active"]))
    got = {k: dev.get(out[k], (sizes[k],), np.int32) for k in SF_KEYS}
    for k in ("sel", "sel_p"):       # entries from nsel on do not exist
        assert np.all(got[k][nsel:] == SENT_I), k
        got[k] = got[k][:nsel]
    return got


def _row_tokens(B, T, counts, rng):
    return np.concatenate([b * T + np.sort(rng.permutation(T)[: counts[b]]) for b in range(B)]).astype(np.int64)


def _sf_cases(B, T):
    """per-row counts of selected tokens, rotated over the rows: none (q_active 0), all, exactly 64, exactly 65 (q_active 1 -> 2), some"""
    C5 = [0, T, min(64, T), min(65, T), max(1, T // 3)]
    return [[C5[(k + b) % 5] for b in range(B)] for k in range(5)]


# T = 72: rows start in the middle of a bitmap word (72 = 2 * 32 + 8) and the last 64-token tile is ragged; tokens per thread of the
# 1024-thread workgroup of a row = ceil(T / 1024): 1 up to T = 1024, 2 at 1032 (516 busy threads), 4 at 4096
@pytest.mark.parametrize("B,T", [(1, 8), (3, 72), (2, 1024), (2, 1032), (1, 4096)])
def test_selected_first(dev, B, T):
    rng = np.random.default_rng(B * 10000 + T)
    n = B * T
    uid = rng.integers(0, 1 << 19, n); tm = rng.integers(0, 4096, n)
    for counts in _sf_cases(B, T):
        toks = _row_tokens(B, T, counts, rng)
        for rope_pos in (None, rng.integers(0, 5000, n)):        # non-monotone positions
            got = _run_selected_first(dev, toks, B, T, uid, tm, rope_pos)
            want = ix.selected_first(toks, B, T, uid, tm, rope_pos)
            for k in SF_KEYS:
                assert np.array_equal(got[k], want[k]), (k, counts, rope_pos is not None)
            # the contract of rsys_debug.h, stated on the outputs themselves
            assert np.array_equal(got["q_active"], [-(-c // 64) for c in counts])
            for b in range(B):
                row = got["slot_p"][b * T:(b + 1) * T]
                assert np.all(row[: counts[b]] >= 0) and np.all(row[counts[b]:] == -1)
            dev.free()


@pytest.mark.parametrize("B,T", [(3, 72), (2, 1032)])
def test_selected_first_identity_order(dev, monkeypatch, B, T):
    """RSYS_TOP_ORDER=0 (parsed at the call): nothing moves, q_active covers the whole row; slot / sel as before"""
    monkeypatch.setenv("RSYS_TOP_ORDER", "0")
    rng = np.random.default_rng(T)
    n = B * T
    uid = rng.integers(0, 1 << 19, n); tm = rng.integers(0, 4096, n); rope_pos = rng.integers(0, 5000, n)
    for counts in _sf_cases(B, T)[:3]:
        toks = _row_tokens(B, T, counts, rng)
        got = _run_selected_first(dev, toks, B, T, uid, tm, rope_pos)
        want = ix.selected_first(toks, B, T, uid, tm, rope_pos, identity=True)
        for k in SF_KEYS:
            assert np.array_equal(got[k], want[k]), (k, counts)
        assert np.array_equal(got["perm"], np.arange(n)) and np.all(got["q_active"] == -(-T // 64))
        dev.free()
    monkeypatch.delenv("RSYS_TOP_ORDER")
    got = _run_selected_first(dev, toks, B, T, uid, tm, rope_pos)          # and back: the switch is read at every call
    assert np.array_equal(got["perm"], ix.selected_first(toks, B, T, uid, tm, rope_pos)["perm"])


def test_selected_first_argument_checks(dev):
    toks = np.array([1, 5, 40], np.int64)
    dbits, dpre = _bitmap_from_union(dev, toks, 64)
    bufs = [dev.put(np.zeros(64), np.int32) for _ in range(11)]
    args = lambda pre, T, cap: (dbits, pre, 1, T, bufs[0], bufs[1], None, bufs[2], bufs[3], cap, *bufs[4:11])
    assert dev.L.rsys_op_selected_first(*args(dpre, 64, 3)) == 0
    assert dev.L.rsys_op_selected_first(*args(dpre, 64, 2)) == ERR_ARG                  # sel / sel_p too small for the three tokens
    assert dev.L.rsys_op_selected_first(*args(dev.put([0, 1], np.int32), 64, 3)) == ERR_ARG   # pre is not the prefix count (it is [0, 2])
    assert dev.L.rsys_op_selected_first(*args(dpre, 4097, 3)) == ERR_ARG                # the launcher's bound on T


# ============================================================================================ row movers
def _D(dt, chunks):
    """columns of a row of `chunks` 16-byte pieces: 1, 64 and 65 are fewer than, exactly and more than one pass of a 64-lane wave"""
    return chunks * (8 if dt == BF16 else 4)


def _vals(rng, shape):
    return rng.integers(-120, 121, shape).astype(np.float32)          # exact in bf16: moved rows compare equal


def _rows(dev, kind, dt, src, src_rows, dst, dst_rows, ld, n, D, map_=None, map_len=0, idx=None, parity=0, count=None, Tseq=0):
    return dev.L.rsys_op_rows(kind, dt, src, src_rows, dst, dst_rows, ld, n, D, map_, map_len, idx, parity, count, Tseq)


@pytest.mark.parametrize("chunks", [1, 64, 65])
@pytest.mark.parametrize("dt", DTYPES)
def test_gather_rows_sel(dev, dt, chunks):
    rng = np.random.default_rng(chunks + dt)
    D = _D(dt, chunks); ld = D + 2 * _D(dt, 1); R = 700
    src = _vals(rng, (R, ld))
    dsrc = dev.put_t(src, dt)
    # n rounded up to 256 is zero-filled, clipped at cap (300 with n = 290: zeros stop at cap); later rows keep the sentinel
    for cap, n in [(512, 0), (512, 1), (512, 255), (512, 256), (512, 257), (512, 512), (300, 290), (300, 300), (300, 1)]:
        sel = rng.integers(0, R, cap)
        ddst = dev.put_t(np.full((cap, D), SENT), dt); dsel = dev.put(sel, np.int32); dn = dev.put([n], np.int32)
        _ok(_rows(dev, 0, dt, dsrc, R, ddst, cap, ld, 0, D, map_=dsel, map_len=cap, count=dn))
        got = dev.get_t(ddst, (cap, D), dt)
        want = ix.gather_rows_sel(np.full((cap, D), SENT, np.float32), src, sel, n)
        assert np.array_equal(got, want), (cap, n)
        z = min(cap, -(-n // 256) * 256)
        assert np.all(got[n:z] == 0) and np.all(got[z:] == SENT), (cap, n)


@pytest.mark.parametrize("chunks", [1, 64, 65])
@pytest.mark.parametrize("dt", DTYPES)
def test_scatter_rows_fill(dev, dt, chunks):
    rng = np.random.default_rng(10 + chunks + dt)
    D = _D(dt, chunks); ld = D + _D(dt, 1); R = 50
    src = _vals(rng, (R, D))
    dsrc = dev.put_t(src, dt)
    # T = 72: q_active 0 visits nothing, 1 the first 64 places, 2 the whole row (64 * 2 > 72: clipped at the row's end)
    for B, T, qa in [(3, 72, [0, 1, 2]), (3, 72, [2, 0, 1]), (1, 64, [1]), (2, 136, [3, 2])]:
        slot_p = rng.integers(-1, R, B * T); slot_p[rng.random(B * T) < 0.3] = -1
        ddst = dev.put_t(np.full((B * T, ld), SENT), dt); dsp = dev.put(slot_p, np.int32); dqa = dev.put(qa, np.int32)
        _ok(_rows(dev, 1, dt, dsrc, R, ddst, B * T, ld, B, D, map_=dsp, map_len=B * T, count=dqa, Tseq=T))
        got = dev.get_t(ddst, (B * T, ld), dt)
        assert np.array_equal(got, ix.scatter_rows_fill(np.full((B * T, ld), SENT, np.float32), src, slot_p, qa, T)), (B, T, qa)
        for b in range(B):
            v = min(T, 64 * qa[b])
            assert np.all(got[b * T + v:(b + 1) * T] == SENT)                              # behind the visited tiles: untouched
            assert np.all(got[b * T: b * T + v, :D][slot_p[b * T: b * T + v] < 0] == 0)    # no selected token at the place: zeros


@pytest.mark.parametrize("chunks", [1, 64, 65])
@pytest.mark.parametrize("dt", DTYPES)
def test_scatter_rows_map(dev, dt, chunks):
    rng = np.random.default_rng(20 + chunks + dt)
    D = _D(dt, chunks); ld = D + 3 * _D(dt, 1)
    for n, rows in [(37, 37), (20, 50), (1, 3)]:                 # a full permutation, a partial map, one row
        src = _vals(rng, (n, D)); m = rng.permutation(rows)[:n]
        ddst = dev.put_t(np.full((rows, ld), SENT), dt)
        _ok(_rows(dev, 2, dt, dev.put_t(src, dt), n, ddst, rows, ld, n, D, map_=dev.put(m, np.int32), map_len=n))
        got = dev.get_t(ddst, (rows, ld), dt)
        assert np.array_equal(got, ix.scatter_rows_map(np.full((rows, ld), SENT, np.float32), src, m)), (n, rows)
        assert np.all(np.delete(got, m, axis=0) == SENT) and np.all(got[:, D:] == SENT)


def _head_setup(rng, P, R, n):
    """P positions (2 P tokens), a slot map onto R compact rows with a third of the tokens outside the set, n distinct positions"""
    slot = np.full(2 * P, -1, np.int64)
    inside = rng.permutation(2 * P)[:R]
    slot[inside] = rng.permutation(R)
    return slot, rng.permutation(P)[:n]


@pytest.mark.parametrize("chunks", [1, 64, 65])
@pytest.mark.parametrize("dt", DTYPES)
def test_gather_rows_and_gather_rows_slot(dev, dt, chunks):
    rng = np.random.default_rng(30 + chunks + dt)
    D = _D(dt, chunks); ld = D + _D(dt, 1); P, R, n = 150, 200, 70
    slot, idx = _head_setup(rng, P, R, n)
    compact = _vals(rng, (R, D)); table = _vals(rng, (2 * P, ld))
    dcomp = dev.put_t(compact, dt); dtab = dev.put_t(table, dt); dslot = dev.put(slot, np.int32); didx = dev.put(idx, np.int32)
    for parity in (0, 1):
        assert (slot[2 * idx + parity] < 0).any() and (slot[2 * idx + parity] >= 0).any()
        ddst = dev.put_t(np.full((n, D), SENT), dt)
        _ok(_rows(dev, 3, dt, dcomp, R, ddst, n, 0, n, D, map_=dslot, map_len=2 * P, idx=didx, parity=parity))
        assert np.array_equal(dev.get_t(ddst, (n, D), dt), ix.gather_rows_slot(compact, slot, idx, parity)), parity     # slot -1: zeros
        ddst = dev.put_t(np.full((n, D), SENT), dt)
        _ok(_rows(dev, 5, dt, dtab, 2 * P, ddst, n, ld, n, D, idx=didx, parity=parity))
        assert np.array_equal(dev.get_t(ddst, (n, D), dt), ix.gather_rows(table, idx, parity, D)), parity


@pytest.mark.parametrize("chunks", [1, 64, 65])
def test_scatter_rows_add_and_scatter_rows_add_slot(dev, chunks):
    rng = np.random.default_rng(40 + chunks)
    D = _D(F32, chunks); ld = D + 8; P, R, n = 150, 200, 70
    slot, idx = _head_setup(rng, P, R, n)
    src = _vals(rng, (n, D))
    compact0 = rng.integers(1, 9, (R, D)).astype(np.float32); table0 = rng.integers(1, 9, (2 * P, ld)).astype(np.float32)   # nonzero: += is not =
    dsrc = dev.put(src, np.float32); dslot = dev.put(slot, np.int32); didx = dev.put(idx, np.int32)
    for parity in (0, 1):
        for npos in (0, 30, n + 130, None):        # *npos of 0, below n, above n; the plain form also without a count
            dnp = dev.put([npos], np.int32) if npos is not None else None
            if npos is not None:
                dc = dev.put(compact0, np.float32)
                _ok(_rows(dev, 4, F32, dsrc, n, dc, R, 0, n, D, map_=dslot, map_len=2 * P, idx=didx, parity=parity, count=dnp))
                assert np.array_equal(dev.get(dc, (R, D), np.float32), ix.scatter_rows_add_slot(compact0, src, slot, idx, parity, npos)), (parity, npos)
            dtb = dev.put(table0, np.float32)
            _ok(_rows(dev, 6, F32, dsrc, n, dtb, 2 * P, ld, n, D, idx=didx, parity=parity, count=dnp))
            assert np.array_equal(dev.get(dtb, (2 * P, ld), np.float32), ix.scatter_rows_add(table0, src, idx, parity, npos)), (parity, npos)
        dev.free()
        dsrc = dev.put(src, np.float32); dslot = dev.put(slot, np.int32); didx = dev.put(idx, np.int32)


def test_rows_argument_checks(dev):
    f = dev.put(np.zeros(64 * 8), np.float32); g = dev.put(np.zeros(64 * 8), np.float32)
    i = dev.put(np.arange(8), np.int32); one = dev.put([1], np.int32); neg = dev.put([-1, 0, 1, 2, 3, 4, 5, 6], np.int32)
    dup = dev.put([3, 3], np.int32); big = dev.put([9], np.int32)
    assert _rows(dev, 2, F32, f, 8, g, 8, 8, 0, 8, map_=i, map_len=8) == ERR_ARG                       # n = 0: a grid of no workgroup
    assert _rows(dev, 2, F32, f, 8, g, 8, 8, 2, 8, map_=dup, map_len=2) == ERR_ARG                     # two rows onto one
    assert _rows(dev, 2, F32, f, 8, g, 8, 8, 2, 6, map_=i, map_len=2) == ERR_ARG                       # a row of 24 bytes
    assert _rows(dev, 2, BF16, f, 8, g, 8, 12, 2, 8, map_=i, map_len=2) == ERR_ARG                     # a bf16 stride of 24 bytes
    assert _rows(dev, 0, F32, f, 8, g, 8, 8, 0, 8, map_=i, map_len=8, count=big) == ERR_ARG            # *count > cap
    assert _rows(dev, 0, F32, f, 4, g, 8, 8, 0, 8, map_=i, map_len=8, count=dev.put([8], np.int32)) == ERR_ARG   # sel names source row 4 .. 7 of 4
    assert _rows(dev, 5, F32, f, 8, g, 8, 8, 5, 8, idx=i, parity=1) == ERR_ARG                         # token 2 * 3 + 1 = 7 is the last: idx 4 is outside
    assert _rows(dev, 5, F32, f, 8, g, 8, 8, 4, 8, idx=neg, parity=0) == ERR_ARG
    assert _rows(dev, 3, F32, f, 2, g, 8, 0, 2, 8, map_=neg, map_len=8, idx=i, parity=1) == ERR_ARG    # slot[3] = 2 names compact row 2 of 2
    assert _rows(dev, 6, BF16, f, 8, g, 8, 8, 2, 8, idx=i, parity=0, count=one) == ERR_ARG             # the adding movers are fp32
    assert _rows(dev, 7, F32, f, 8, g, 8, 8, 2, 8, idx=i) == ERR_ARG


# ============================================================================================ column sums and casts
def _exact(rng, shape):
    """small integers times 2^-3: every column sum of up to 2^17 rows is exact in fp32 whatever the order"""
    return rng.integers(-8, 9, shape, dtype=np.int8).astype(np.float32) * np.float32(0.125)


def _ties(rng, shape):
    """exact bf16 ties (odd 9-bit integers times 2^-3: the dropped bit is the only one set), both signs, +0 and -0 and a few plain values;
    still integers times 2^-3 below 2^6, so sums stay exact"""
    m = (2 * rng.integers(128, 256, shape) + 1).astype(np.float32)          # 257 .. 511, odd
    x = m * np.where(rng.random(shape) < 0.5, -1, 1).astype(np.float32) * np.float32(0.125)
    r = rng.random(shape)
    x[r < 0.1] = 0.0; x[(r >= 0.1) & (r < 0.2)] = -0.0; x[(r >= 0.2) & (r < 0.3)] = 1.5
    return x


def _colsum_call(dev, kind, det, dsrc, ld, rows, D, init, dst_shape=None, ldt=0):
    dcs = dev.put(init, np.float32)
    ddst = dev.put(np.full(dst_shape, SENT_H), np.uint16) if dst_shape is not None else None
    _ok(dev.L.rsys_op_colsum(kind, int(det), dsrc, ld, rows, D, dcs, ddst, ldt))      # (det: RSYS_ERR_STATE unless the partial-sum branch ran)
    return dev.get(dcs, (D,), np.float32), (dev.get(ddst, dst_shape, np.uint16) if dst_shape is not None else None)


def _colsum_modes(dev, kind, dsrc, ld, rows, D, init, dst_shape=None, ldt=0):
    """default mode, then deterministic mode twice (bitwise equal); returns [(colsum, dst)] of the three launches"""
    res = [_colsum_call(dev, kind, det, dsrc, ld, rows, D, init, dst_shape, ldt) for det in (0, 1, 1)]
    assert np.array_equal(res[1][0].view(np.uint32), res[2][0].view(np.uint32))
    return res


# rows per workgroup = max(64, ceil(rows / 512)): 1, 63, 64 are one workgroup row, 65 two (the second with one row), 33000 gives 65 rows per
# workgroup and 508 of them (deterministic: the two-stage sum of more than 64 partials); 300 columns: a ragged second 256-column block
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 33000])
def test_colsum_add_exact(dev, rows):
    rng = np.random.default_rng(rows)
    for cols in (8, 256, 300):
        ld = 2 * cols
        src = _exact(rng, (rows, ld))
        init = rng.integers(-5, 6, cols).astype(np.float32)                 # dst pre-filled: the kernel adds
        dsrc = dev.put(src, np.float32)
        want = init.astype(np.float64) + ix.colsum(src[:, cols:])[0]        # the odd half of interleaved rows, as model_backward.hip calls it
        for cs, _ in _colsum_modes(dev, 0, _off(dsrc, cols * 4), ld, rows, cols, init):
            assert np.array_equal(cs, want), (rows, cols)
        dev.free()


# row lanes per workgroup = 1024 / (D / 4): D = 4, 64, 256, 1024 give 1024, 64, 16, 4; rows per workgroup = max(32, ceil(rows / 512)):
# 33 starts a second workgroup, 16400 gives 33 rows per workgroup on 497 workgroups.  A thread runs its four-row unrolled loop while
# four more rows of its lane fit: (D 1024, rows 22) runs it once for rows 0 .. 15 and the tail for 16 .. 21; (1024, 32) twice without a
# tail; (256, 30720) = 60 rows per workgroup on 16 lanes: lanes 0 .. 11 unrolled, all lanes a tail
CAST_CASES = [(D, r) for D in (4, 64, 256, 1024) for r in (1, 31, 32, 33, 16400)] + [(1024, 22), (256, 30720)]


@pytest.mark.parametrize("D,rows", CAST_CASES)
def test_cast_colsum_exact(dev, D, rows):
    rng = np.random.default_rng(D * 7 + rows)
    inputs = [_exact(rng, (rows, D))] + ([_ties(rng, (rows, D))] if rows <= 64 else [])
    for src in inputs:
        init = rng.integers(-5, 6, D).astype(np.float32)
        want = init.astype(np.float64) + ix.colsum(src)[0]
        want_bits = ix.bf16_bits(src)
        for cs, dst in _colsum_modes(dev, 1, dev.put(src, np.float32), D, rows, D, init, (rows, D)):
            assert np.array_equal(cs, want), (D, rows)
            assert np.array_equal(dst, want_bits), (D, rows)                # bit for bit: nearest even, signed zeros kept
        dev.free()


# a workgroup owns max(1, ceil(ceil(rows / 64) / 2048)) 64-row chunks: one up to 131072 rows; 131136 rows = 2049 chunks gives two per
# workgroup (1025 workgroups, the last with one chunk)
@pytest.mark.parametrize("D,rows", [(D, r) for D in (64, 192) for r in (1, 63, 64, 65, 200)] + [(64, 131136)])
def test_cast_transpose_colsum_exact(dev, D, rows):
    rng = np.random.default_rng(D + rows)
    r64 = -(-rows // 64) * 64
    ldt = r64 + 72                                                          # > rows rounded up to 64, a multiple of 8
    inputs = [_exact(rng, (rows, D))] + ([_ties(rng, (rows, D))] if rows <= 200 else [])
    for src in inputs:
        init = rng.integers(-5, 6, D).astype(np.float32)
        want = init.astype(np.float64) + ix.colsum(src)[0]
        want_t = ix.cast_transpose(src, np.full((D, ldt), SENT_H, np.uint16))
        for cs, dstT in _colsum_modes(dev, 2, dev.put(src, np.float32), D, rows, D, init, (D, ldt), ldt):
            assert np.array_equal(cs, want), (D, rows)
            assert np.array_equal(dstT, want_t), (D, rows)
            assert not dstT[:, rows:r64].any() and np.all(dstT[:, r64:] == SENT_H)     # zero K-padding up to 64, untouched behind it
        dev.free()


def _gamma(c):
    return c * U / (1 - c * U)


def _float_case(dev, kind, rows, D, ld, c, dst_shape=None, ldt=0):
    """random floats: |fp32 sum - fp64 sum| <= gamma_c sum |terms|, c = roundings on the longest chain of the kernel's summation"""
    rng = np.random.default_rng(rows + D)
    src = (rng.standard_normal((rows, ld)) * np.exp(rng.uniform(-3, 3, (rows, 1)))).astype(np.float32)
    init = rng.standard_normal(D).astype(np.float32)
    s, mag = ix.colsum(src[:, :D])
    for cs, _ in _colsum_modes(dev, kind, dev.put(src, np.float32), ld, rows, D, init, dst_shape, ldt):
        err = np.abs(cs.astype(np.float64) - (init + s)) - _gamma(c) * (np.abs(init) + mag)
        assert err.max() <= 0, (kind, float(err.max()))


def test_colsum_add_random_floats(dev):
    # 5000 rows: 64 rows per workgroup, 79 partials.  Chain: a thread adds its 64 rows in order (63 roundings), then either 79 atomics onto
    # dst in any order (79) or, deterministic, 32 partials per stage-one sum (31), 3 stage sums (2) and the add onto dst (1): c <= 63 + 79
    _float_case(dev, 0, 5000, 300, 304, 63 + 79)


def test_cast_colsum_random_floats(dev):
    # D = 256: 16 row lanes; 3000 rows: 32 rows per workgroup, 94 partials.  Chain: a thread adds its 2 rows (1), lanes 2 .. 15 are added
    # onto two LDS rows one pair at a time (7), the two rows are added (1), then 94 atomics (94) or the ordered sum (31 + 2 + 1): c <= 9 + 94
    _float_case(dev, 1, 3000, 256, 256, 9 + 94, (3000, 256))


def test_cast_transpose_colsum_random_floats(dev):
    # 5000 rows, D = 64: 79 chunks, one per workgroup.  Chain: a thread adds its 4 rows of the chunk (3), 16 row groups are added in LDS in
    # order (15), then 79 atomics (79) or the ordered sum (31 + 2 + 1): c <= 18 + 79
    _float_case(dev, 2, 5000, 64, 64, 18 + 79, (64, 5056 + 8), 5056 + 8)


def test_colsum_argument_checks(dev):
    f = dev.put(np.zeros(64 * 64), np.float32); cs = dev.put(np.zeros(64), np.float32); h = dev.put(np.zeros(64 * 128), np.uint16)
    assert dev.L.rsys_op_colsum(3, 0, f, 64, 8, 64, cs, h, 64) == ERR_ARG
    assert dev.L.rsys_op_colsum(0, 0, f, 8, 8, 64, cs, None, 0) == ERR_ARG               # ld < cols
    assert dev.L.rsys_op_colsum(0, 0, f, 64, 0, 64, cs, None, 0) == ERR_ARG              # no rows: a grid of no workgroup
    assert dev.L.rsys_op_colsum(1, 0, f, 64, 8, 64, cs, None, 0) == ERR_ARG              # the cast forms take dst
    assert dev.L.rsys_op_colsum(1, 0, f, 12, 8, 12, cs, h, 0) == ERR_ARG                 # D / 4 = 3 does not divide 1024
    assert dev.L.rsys_op_colsum(2, 0, f, 64, 65, 64, cs, h, 120) == ERR_ARG              # ldt < 128 = 65 rounded up to 64
    assert dev.L.rsys_op_colsum(2, 0, f, 64, 8, 64, cs, h, 68) == ERR_ARG                # ldt % 8


# ============================================================================================ batched transpose
def _run_transpose(dev, jobs, rng):
    """jobs: (rows, cols, ld_src, ld_dst); one launch; returns [(dst read back, expectation)]"""
    n = len(jobs)
    srcs = [rng.integers(0, 1 << 16, (r, ls)).astype(np.uint16) for r, c, ls, ld in jobs]
    dsrc = [dev.put(s, np.uint16) for s in srcs]
    ddst = [dev.put(np.full((c, ld), SENT_H), np.uint16) for r, c, ls, ld in jobs]
    ps = (C.c_void_p * n)(*[p.value for p in dsrc]); pd = (C.c_void_p * n)(*[p.value for p in ddst])
    rows = (C.c_int32 * n)(*[j[0] for j in jobs]); cols = (C.c_int32 * n)(*[j[1] for j in jobs])
    ls = (C.c_int64 * n)(*[j[2] for j in jobs]); ld = (C.c_int64 * n)(*[j[3] for j in jobs])
    _ok(dev.L.rsys_op_transpose_bf16(n, ps, pd, rows, cols, ls, ld))
    return [(dev.get(ddst[k], (c, l), np.uint16), ix.transpose(np.full((c, l), SENT_H, np.uint16), srcs[k], r, c))
            for k, (r, c, _, l) in enumerate(jobs)]


def test_transpose_bf16_three_shapes_in_one_launch(dev):
    # the grid comes from the maxima (129 rows, 100 columns: 3 x 2 tiles per job): the 8 x 8 job returns early in five of six workgroups,
    # 70 x 100 has ragged tiles on both sides; ld_src > cols and ld_dst > rows: the padding keeps the sentinel
    jobs = [(70, 100, 104, 72), (8, 8, 16, 16), (129, 64, 72, 136)]
    for (got, want), (r, c, _, l) in zip(_run_transpose(dev, jobs, np.random.default_rng(1)), jobs):
        assert np.array_equal(got, want), (r, c)
        assert np.all(got[:, r:] == SENT_H)


def test_transpose_bf16_sixty_four_jobs(dev):
    rng = np.random.default_rng(2)
    jobs = []
    for k in range(64):
        r, c = int(rng.integers(1, 80)), int(rng.integers(1, 80))
        jobs.append((r, c, -(-c // 8) * 8 + 8 * (k % 2), -(-r // 8) * 8 + 8 * (k % 3)))
    for got, want in _run_transpose(dev, jobs, rng):
        assert np.array_equal(got, want)


def test_transpose_bf16_argument_checks(dev):
    s = dev.put(np.zeros(64 * 64), np.uint16); d = dev.put(np.zeros(64 * 64), np.uint16)

    def call(n, rows, cols, ls, ld, src=s, dst=d):
        n_arr = max(n, 1)
        return dev.L.rsys_op_transpose_bf16(n, (C.c_void_p * n_arr)(*[src.value] * n_arr), (C.c_void_p * n_arr)(*[dst.value] * n_arr),
                                            (C.c_int32 * n_arr)(*[rows] * n_arr), (C.c_int32 * n_arr)(*[cols] * n_arr),
                                            (C.c_int64 * n_arr)(*[ls] * n_arr), (C.c_int64 * n_arr)(*[ld] * n_arr))
    assert call(1, 8, 8, 8, 8) == 0
    assert call(0, 8, 8, 8, 8) == ERR_ARG and call(65, 8, 8, 8, 8) == ERR_ARG
    assert call(1, 8, 8, 12, 8) == ERR_ARG and call(1, 8, 8, 8, 12) == ERR_ARG           # row strides of 24 bytes
    assert call(1, 8, 9, 8, 8) == ERR_ARG and call(1, 9, 8, 8, 8) == ERR_ARG             # ld_src < cols, ld_dst < rows
    assert call(1, 8, 8, 8, 8, src=_off(s, 2)) == ERR_ARG                                # a matrix that is not 16-byte aligned
