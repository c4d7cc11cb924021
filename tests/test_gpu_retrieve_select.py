"""GPU: the selection stage of retrieve.hip on its own, every assertion exact.  rsys_op_topk_window (win_select_step / win_hist_pass /
win_count / win_compact / win_sort) and rsys_op_topk (select_step / hist_pass / count / compact / sort_out) against the stable numpy
sort of tests/_retrieve_np.py, on score populations built for the branches of the radix select: windows are chosen per row from the
tie-block edges of the reference ordering, and the (threshold key, need) pair of both rank bounds that the hook returns is compared with
a numpy restatement of the select, so a test that names a branch also shows that the device took it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _retrieve_np as rn  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_ARG = -1                     # RSYS_ERR_ARG
WIN = rn.RT_WIN
KINDS = ["random", "equal", "ulp", "zeros", "special", "digit_edges"]


# ---------------------------------------------------------------- device plumbing
class _Dev:
    """device buffers of one test, freed together"""

    def __init__(self):
        from recommendersystem_amd._lib import check, lib
        self.L, self.check, self.ptrs = lib(), check, []

    def alloc(self, nbytes, fill=None):
        p = C.c_void_p()
        self.check(self.L.rsys_dev_alloc(C.byref(p), max(int(nbytes), 4)))
        self.ptrs.append(p)
        if fill is not None:
            self.check(self.L.rsys_dev_memset(p, fill, max(int(nbytes), 4)))
        return p

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        self.check(self.L.rsys_dev_h2d(p, a.ctypes.data, a.nbytes))
        return p

    def get(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        self.check(self.L.rsys_dev_d2h(out.ctypes.data, p, out.nbytes))
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.L.rsys_dev_free(p)


def _padded(scores, ld):
    rows, V = scores.shape
    host = np.full((rows, V if ld is None else ld), np.nan, np.float32)      # NaN in the padding columns
    host[:, :V] = scores
    return host


class _Windows:
    """score rows uploaded once; window(start, len) runs rsys_op_topk_window on them"""

    def __init__(self, dev, scores, ld=None):
        self.d, self.rows, self.V = dev, scores.shape[0], scores.shape[1]
        self.ld = self.V if ld is None else ld
        self.p = dev.put(_padded(scores, ld))
        r = self.rows
        self.out = [dev.alloc(r * WIN * 4), dev.alloc(r * WIN * 4), dev.alloc(r * 4), dev.alloc(r * 4), dev.alloc(r * 16)]

    def window(self, start, length):
        d, r = self.d, self.rows
        start = np.ascontiguousarray(np.broadcast_to(np.asarray(start, np.int64), (r,)))
        length = np.ascontiguousarray(np.broadcast_to(np.asarray(length, np.int32), (r,)))
        o = self.out
        d.check(d.L.rsys_op_topk_window(self.p, self.ld, r, self.V, start.ctypes.data, length.ctypes.data, o[0], o[1], o[2], o[3], o[4]))
        return (d.get(o[0], (r, WIN), np.int32), d.get(o[1], (r, WIN), np.float32), d.get(o[2], r, np.int32), d.get(o[3], r, np.int32),
                d.get(o[4], (r, 2, 2), np.int32))


def _op_topk(scores, k, ld=None):
    rows, V = scores.shape
    with _Dev() as d:
        p = d.put(_padded(scores, ld))
        o = [d.alloc(rows * k * 4), d.alloc(rows * k * 4), d.alloc(rows * 4)]
        d.check(d.L.rsys_op_topk(p, V if ld is None else ld, rows, V, k, o[0], o[1], o[2]))
        return d.get(o[0], (rows, k), np.int32), d.get(o[1], (rows, k), np.float32), d.get(o[2], rows, np.int32)


# ---------------------------------------------------------------- references, computed once per population
_REF = {}


def _population(kind, rows, V):
    """(scores, per-row ordering, per-row named windows) of a population; computed once, shared, never written to."""
    key = (kind, rows, V)
    if key not in _REF:
        rng = np.random.default_rng(7 * V + rows + 1000 * KINDS.index(kind))
        x = rn._rows(kind, rows, V, rng)
        x.setflags(write=False)
        orders = [rn.full_order(row) for row in x]
        _REF[key] = (x, orders, [rn.named_windows(row, o) for row, o in zip(x, orders)])
    return _REF[key]


def _check_window(x, orders, start, length, got, where):
    ids, vals, counts, totals, bounds = got
    start = np.broadcast_to(np.asarray(start, np.int64), (x.shape[0],))
    length = np.broadcast_to(np.asarray(length, np.int32), (x.shape[0],))
    for r in range(x.shape[0]):
        e_ids, e_vals, e_count, e_total = rn.expect_window(x[r], orders[r], int(start[r]), int(length[r]))
        w = (where, r, int(start[r]), int(length[r]))
        assert (counts[r], totals[r]) == (e_count, e_total), (w, counts[r], totals[r], e_count, e_total)
        assert ids[r].tobytes() == e_ids.tobytes(), w
        assert vals[r].tobytes() == e_vals.tobytes(), w
        e_b = rn.expect_bounds(x[r], int(start[r]), int(length[r]))
        assert np.array_equal(bounds[r], e_b), (w, [hex(int(v) & 0xffffffff) for v in bounds[r].ravel()], [hex(int(v) & 0xffffffff) for v in e_b.ravel()])


def _assert_branch(name, row, b):
    """the branch a named window is for, read off the device's bounds (end, start) = b"""
    (te, ne), (ts, ns) = [(int(t) & 0xffffffff, int(n)) for t, n in b]
    keys = rn.score_keys(row)
    between = ((keys > te) & (keys < ts)).any()
    if name == "first":
        assert (ts, ns) == (0xffffffff, 0)
    elif name == "inside_largest":
        assert te == ts and 0 < ns < ne                              # `same`, both exact, need_start > 0
    elif name == "block_start":
        assert rn.is_between_form(ts, ns)
    elif name == "block_end":
        assert rn.is_between_form(te, ne)
    elif name == "real_key_at_T":
        assert te == ts and rn.is_between_form(ts, ns) and 0 < ne < (keys == te).sum()   # `same` with mixed forms on a real key
    elif name == "two_blocks":
        assert te < ts and ne > 0 and ns > 0 and not between          # W == 0: the two tie tails only
    elif name == "three_blocks":
        assert te < ts and between
    elif name in ("at_total", "past_total", "far_past"):
        T = 0 if (keys != 0).any() else 0xffffffff                    # (c == total: every key is above 0; no admissible key: c == 0)
        assert (te, ne, ts, ns) == (T, 0, T, 0)
    elif name in ("last_five", "exactly_1024_left", "only_1023_left"):
        assert (te, ne) == (0, 0)


SHAPES = [(V, 5) for V in (1, 37, 64, 65, 1023, 1024, 1025, 4097)] + [(119999, 8)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V,rows", SHAPES)
def test_window_named(kind, V, rows):
    """Every named window, one call per name with each row's own (start, len), then one call in which neighbouring rows take different
    names.  A row without such a window (too few blocks or ranks) takes rank 0, len 1."""
    x, orders, named = _population(kind, rows, V)
    if kind == "digit_edges" and V >= 1025:
        assert all(set(W) == set(rn.WINDOW_NAMES) for W in named)
    with _Dev() as d:
        dev = _Windows(d, x)
        for name in rn.WINDOW_NAMES:
            sl = [W.get(name, (0, 1)) for W in named]
            start, length = [s for s, _ in sl], [n for _, n in sl]
            got = dev.window(start, length)
            _check_window(x, orders, start, length, got, (kind, V, name))
            for r, W in enumerate(named):
                if name in W:
                    _assert_branch(name, x[r], got[4][r])
        sl = [named[r].get(rn.WINDOW_NAMES[(3 * r + 1) % len(rn.WINDOW_NAMES)], (r, 1 + r)) for r in range(rows)]
        start, length = [s for s, _ in sl], [n for _, n in sl]
        _check_window(x, orders, start, length, dev.window(start, length), (kind, V, "mixed"))
    if kind == "special":                                             # the last row is all -inf: total 0, every window empty
        assert orders[-1].size == 0 and (got[2][-1], got[3][-1]) == (0, 0) and (got[0][-1] == -1).all()


def test_window_row_stride_with_nan_padding():
    x, orders, named = _population("digit_edges", 5, 1000)
    with _Dev() as d:
        dev = _Windows(d, x, ld=1031)
        for name in ("inside_largest", "real_key_at_T", "two_blocks", "three_blocks", "last_five", "at_total"):
            sl = [W.get(name, (0, 1)) for W in named]
            start, length = [s for s, _ in sl], [n for _, n in sl]
            _check_window(x, orders, start, length, dev.window(start, length), ("ld", name))


def test_window_rows_without_an_admissible_item():
    """Rows of NaN, of -inf and of both next to a row with one admissible item: totals 0 / 0 / 0 / 1, the padding everywhere else."""
    x = np.full((4, 65), np.nan, np.float32)
    x[1] = -np.inf
    x[2, ::2] = -np.inf
    x[3, 1::2] = -np.inf
    x[3, 64] = -0.0
    orders = [rn.full_order(row) for row in x]
    assert [o.size for o in orders] == [0, 0, 0, 1]
    with _Dev() as d:
        dev = _Windows(d, x)
        for start, length in ((0, 1), (0, 1024), (1, 5), ([0, 1, 2 ** 40, 0], [1, 2, 3, 4])):
            _check_window(x, orders, start, length, dev.window(start, length), ("none", start))
    for k in (1, 65):
        _check_topk(x, k, ("none", k))


def test_window_300_groups_in_one_launch():
    rng = np.random.default_rng(300)
    x = np.concatenate([rn._rows(kind, 50, 37, rng) for kind in KINDS])
    orders = [rn.full_order(row) for row in x]
    named = [rn.named_windows(row, o) for row, o in zip(x, orders)]
    sl = [named[r].get(rn.WINDOW_NAMES[r % len(rn.WINDOW_NAMES)], (r % 37, 1 + r % 40)) for r in range(300)]
    start, length = [s for s, _ in sl], [n for _, n in sl]
    with _Dev() as d:
        _check_window(x, orders, start, length, _Windows(d, x).window(start, length), "300 rows")


@pytest.mark.parametrize("kind", ["ulp", "digit_edges"])
def test_window_tiles_make_the_whole_ordering(kind):
    x, orders, _ = _population(kind, 3, 9500)
    tiles = []
    with _Dev() as d:
        dev = _Windows(d, x)
        for s0 in range(0, 9500 + WIN, WIN):
            got = dev.window(s0, WIN)
            _check_window(x, orders, s0, WIN, got, (kind, "tile", s0))
            tiles.append(got)
    for r in range(3):
        ids = np.concatenate([t[0][r, :t[2][r]] for t in tiles])
        vals = np.concatenate([t[1][r, :t[2][r]] for t in tiles])
        assert ids.tobytes() == orders[r].tobytes()
        assert vals.tobytes() == (x[r][orders[r]] + np.float32(0)).tobytes()


# ---------------------------------------------------------------- rsys_op_topk at the edges of its tiles
def _check_topk(scores, k, where):
    ids, vals, counts = _op_topk(scores, k)
    for r in range(scores.shape[0]):
        e_ids, e_vals = rn._expect_topk(scores[r], k)
        n = e_ids.size
        assert counts[r] == n, (where, r, counts[r], n)
        assert ids[r, :n].tobytes() == e_ids.tobytes(), (where, r)
        assert vals[r, :n].tobytes() == e_vals.tobytes(), (where, r)
        assert (ids[r, n:] == -1).all() and np.isneginf(vals[r, n:]).all(), (where, r)


TOPK_KS = [1, 2, 3, 63, 64, 65, 1000, 1023, 1024, 1025, 4097, 8191, 8192]


@pytest.mark.parametrize("kind", ["random", "ulp", "digit_edges"])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 1023, 1024, 1025, 4097, 8193])
def test_topk_tile_edges_and_admissible_counts(kind, V):
    """Rows 0-2 are the population; rows 3.. have -inf planted so that 0, 1, k - 1, k and k + 1 entries stay admissible."""
    x, _, _ = _population(kind, 8, V)
    rng = np.random.default_rng(V)
    for k in sorted({min(k, V) for k in TOPK_KS}):
        s = x.copy()
        for r, adm in zip(range(3, 8), (0, 1, k - 1, k, k + 1)):
            adm = min(max(adm, 0), V)
            s[r, rng.permutation(V)[adm:]] = -np.inf
            assert int((s[r] > -np.inf).sum()) == adm
        _check_topk(s, k, (kind, V, k))


@pytest.mark.parametrize("kind", ["ulp", "random", "ulp_tail"])
def test_topk_compact_prefix_loops_twice(kind):
    """V = 300001 is 293 workgroups: compact_kernel's prefix over the earlier workgroups' counts takes a second trip of its 256 threads.
    In `ulp` the first 8192 of the 60000 best-valued items all sit in the first 41 workgroups, so the slots of workgroups 257.. are never
    used; `random` spreads the selected items over every workgroup, and `ulp_tail` keeps the best value only behind item 280000 (the
    4000 keys above the threshold are all in workgroups 273.., the ties of the next value start at item 0)."""
    x, _, _ = _population("ulp" if kind == "ulp_tail" else kind, 1, 300001)
    if kind == "ulp_tail":
        x = x.copy()
        head = x[0, :280000]
        head[head == x.max()] = x.min()
        assert 0 < int((x[0] == x.max()).sum()) < 8192
    _check_topk(x, 8192, kind)


def test_topk_inf_next_to_the_largest_float():
    big = np.finfo(np.float32).max
    x = np.tile(np.array([big, np.inf, big, -big, np.inf, -np.inf, np.nextafter(big, np.float32(0)), 0.0], np.float32), (2, 130))[:, :1037]
    x = np.ascontiguousarray(x)
    for k in (1, 2, 259, 260, 261, 600, 1037):
        _check_topk(x, k, ("inf", k))
    with _Dev() as d:
        orders = [rn.full_order(row) for row in x]
        dev = _Windows(d, x)
        for start, length in ((0, 1), (255, 10), (259, 2), (260, 1024)):
            _check_window(x, orders, start, length, dev.window(start, length), ("inf", start))


# ---------------------------------------------------------------- both hooks: reproducible, argument errors touch nothing
def test_same_call_twice_gives_the_same_bytes():
    x, orders, named = _population("digit_edges", 5, 4097)
    sl = [W["three_blocks"] for W in named]
    start, length = [s for s, _ in sl], [n for _, n in sl]
    with _Dev() as d:
        dev = _Windows(d, x)
        a, b = dev.window(start, length), dev.window(start, length)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))
    a, b = _op_topk(x, 1025), _op_topk(x, 1025)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


def test_argument_errors_leave_the_outputs_alone():
    x = np.zeros((2, 16), np.float32)
    with _Dev() as d:
        p = d.put(x)
        sizes = [2 * WIN * 4, 2 * WIN * 4, 8, 8, 32]
        o = [d.alloc(n, fill=0x5a) for n in sizes]

        def untouched():
            return all((d.get(q, n, np.uint8) == 0x5a).all() for q, n in zip(o, sizes))

        def window(rows, V, ld, start, length):
            start, length = np.array(start, np.int64), np.array(length, np.int32)
            return d.L.rsys_op_topk_window(p, ld, rows, V, start.ctypes.data, length.ctypes.data, *o)

        assert window(2, 16, 16, [0, 0], [1, 0]) == ERR_ARG            # len < 1
        assert window(2, 16, 16, [0, 0], [1025, 1]) == ERR_ARG         # len > 1024
        assert window(2, 16, 16, [0, -1], [1, 1]) == ERR_ARG           # start < 0
        assert window(0, 16, 16, [0, 0], [1, 1]) == ERR_ARG
        assert window(65536, 16, 16, [0] * 65536, [1] * 65536) == ERR_ARG
        assert window(2, 0, 16, [0, 0], [1, 1]) == ERR_ARG
        assert window(2, 16, 15, [0, 0], [1, 1]) == ERR_ARG            # ld < V
        st, ln = np.zeros(2, np.int64), np.ones(2, np.int32)
        assert d.L.rsys_op_topk_window(p, 16, 2, 16, st.ctypes.data, ln.ctypes.data, o[0], None, o[2], o[3], o[4]) == ERR_ARG
        assert d.L.rsys_op_topk_window(p, 16, 2, 16, None, ln.ctypes.data, *o) == ERR_ARG
        for rows, V, k in ((0, 16, 1), (65536, 16, 1), (2, 16, 0), (2, 16, 17), (2, 0, 1)):
            assert d.L.rsys_op_topk(p, 16, rows, V, k, o[0], o[1], o[2]) == ERR_ARG
        assert d.L.rsys_op_topk(p, 15, 2, 16, 1, o[0], o[1], o[2]) == ERR_ARG
        assert untouched()
        assert window(2, 16, 16, [0, 0], [1, 1]) == 0 and not untouched()      # the same buffers are written by a valid call
