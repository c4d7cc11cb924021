"""CPU: the host side of ranking and reranking (rsys_rank_request): the numpy restatement's argmax and max conventions, the request
packing of serve.rank_arrays, "{m}.related" loading through julia_csc, and the pagination arithmetic of serve.render."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_rank_np as rk  # noqa: E402


def test_zero_penalties_give_a_stable_descending_order():
    rng = np.random.default_rng(1)
    for n in (1, 5, 64, 300):
        r = rng.integers(-4, 4, n).astype(np.float32)
        r[rng.random(n) < 0.2] = -0.0
        G = rng.standard_normal((n, n)).astype(np.float32)
        pairs = rng.random((n, n)) < 0.1
        flags = rng.random(n) < 0.2
        got = rk.reranking_given(r, G, pairs, flags, n, 0.9, 0.0, 0.0, 0.0)
        want = np.lexsort((np.arange(n), -rk.isless_key(r).astype(np.int64))).tolist()   # (+0.0 above -0.0, as isless orders them)
        assert got == want


def test_isless_order_and_julia_max():
    x = np.array([np.nan, np.inf, 1.0, 0.0, -0.0, -1.0, -np.inf], np.float32)
    k = rk.isless_key(x)
    assert (np.diff(k[::-1].astype(np.int64)) > 0).all()
    assert rk.jl_argmax(np.array([-0.0, 0.0, 0.0], np.float32)) == 1
    assert rk.jl_argmax(np.array([1.0, np.nan, np.nan], np.float32)) == 1
    m = rk.jl_max(np.array([-0.0, 0.0, np.nan, 1.0], np.float32), np.array([0.0, -0.0, 1.0, np.nan], np.float32))
    assert not np.signbit(m[0]) and not np.signbit(m[1]) and np.isnan(m[2]) and np.isnan(m[3])


def test_repeated_picks_once_the_finite_scores_run_out():
    r = np.array([-np.inf, 2.0, -np.inf, 1.0], np.float32)
    picks = rk.reranking_given(r, np.zeros((4, 4), np.float32), np.zeros((4, 4), bool), np.zeros(4, bool), 6, 1.0, 0.0, 0.0, 0.0)
    assert picks == [1, 3, 0, 0]


def _related():
    # column c holds rows: 0 -> {1, 2}, 1 -> {0}, 2 -> {} , 3 -> {3 (diagonal), 4 (stored zero)}, 4 -> {2}
    indptr = np.array([0, 2, 3, 3, 5, 6], np.int64)
    indices = np.array([1, 2, 0, 3, 4, 2], np.int32)
    data = np.array([1.0, 0.5, 2.0, 1.0, 0.0, 1.0], np.float32)
    return indptr, indices, data, (5, 5)


def test_request_packing_and_related_flags():
    from recommendersystem_amd import serve
    u0 = {"user": {"items": [dict(medium=0, matchedid=0, status=7), dict(medium=0, matchedid=0, status=3),   # completed, then deleted
                             dict(medium=1, matchedid=4, status=7),                                        # other medium
                             dict(medium=0, matchedid=4, status=5)]},                                      # planned
          "embeds": {"0.retrieval": np.ones(4, np.float32), "0.ranking": np.arange(3, dtype=np.float32)}}
    u1 = {"user": {"items": [dict(medium=0, matchedid=1, status=3)]},
          "embeds": {"0.retrieval": np.zeros(4, np.float32), "0.ranking": np.ones(3, np.float32)}}
    st = dict(medium=0, users=[u0, u1], penalties=dict(decay=0.5, mmr_penalty=0.1, same_series_penalty=0.2, related_penalty=0.3))
    idxs = [np.array([2, 0, 1], np.int32)]
    q, group, rm, hist, pen = serve.rank_arrays([st], idxs)
    assert q.shape == (2, 4) and group.tolist() == [0, 0]
    assert hist == [[(0, 0, 7), (0, 0, 3), (1, 4, 7), (0, 4, 5)], [(0, 1, 3)]]        # every entry, in list order
    assert [x.tolist() for x in rm] == [[0, 1, 2], [1, 1, 1]]
    assert pen.tolist() == [[0.5, np.float32(0.1), np.float32(0.2), np.float32(0.3)]]
    flags = rk.related_flags(_related(), idxs[0], st["users"], 0)
    assert flags.tolist() == [True, False, True]      # item 0's column (rows 1, 2); the deleted entry of item 0 does not undo it
    P = rk.pair_matrix(_related(), np.array([3, 4, 2], np.int32))
    assert P.tolist() == [[True, False, False], [False, False, False], [False, True, False]]   # diagonal kept, stored zero dropped


def test_related_through_julia_csc():
    from recommendersystem_amd import serve
    calls = []

    class Fake:
        def set_related(self, m, csc):
            calls.append((m, csc))

    ip, ix, d, shape = _related()
    jl = {"colptr": ip + 1, "rowval": ix + 1, "nzval": d, "m": 5, "n": 5}
    serve.load_ranking_tables(Fake(), {"1.related": jl, "0.dependencies": None})
    assert len(calls) == 1 and calls[0][0] == 1
    ip2, ix2, d2, shape2 = calls[0][1]
    assert np.array_equal(ip2, ip) and np.array_equal(ix2, ix) and np.array_equal(d2, d) and shape2 == (5, 5)


def test_pagination_arithmetic():
    from recommendersystem_amd import serve
    w = serve.page_window
    assert w(5000, {"offset": 0, "limit": 25}) == (0, 1000, 1, 25)               # 1024 - 1024 % 25 = 1000 per ranked slice
    assert w(5000, {"offset": 1000, "limit": 25}) == (1000, 2000, 1, 25)
    assert w(5000, {"offset": 990, "limit": 25}) == (0, 1000, 991, 1015)         # the page runs past the slice, as in render.jl
    assert w(1500, {"offset": 1475, "limit": 25}) == (1000, 1500, 476, 500)      # last slice clamped to the retrieved list
    assert w(1490, {"offset": 1475, "limit": 25}) == (1000, 1490, 476, 490)      # last page clamped
    assert w(100, {"offset": 100, "limit": 10}) is None                           # offset >= total: empty page
    assert w(100, {"offset": 99, "limit": 10}) == (0, 100, 100, 100)
    assert w(3000, {"offset": 2048, "limit": 1024}) == (2048, 3000, 1, 952)
