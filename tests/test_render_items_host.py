"""CPU: the host side of rsys_retrieve_window / rsys_render_items.  The literal restatement of render.jl for a state without users
(tests/_render_items_np.py) agrees with the vectorised oracle the GPU tests use; the window arithmetic from exact totals agrees
with serve.page_window; the Python wrappers validate their arguments before anything reaches the library."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_items_np as ri  # noqa: E402
import _render_rank_np as rk  # noqa: E402
import _render_retrieval_np as rr  # noqa: E402

V = (300, 200)


def _states(rng, which):
    """user-less states of both media: no selection, same-medium, cross-medium, a duplicate, a selection that sums to zero"""
    pen = dict(decay=0.9, mmr_penalty=0.25, same_series_penalty=0.5, related_penalty=0.5)
    out = []
    for m in (0, 1):
        plus, minus = np.flatnonzero(which[m] == 0), np.flatnonzero(which[m] == 1)
        sels = [[], [(m, 5)], [(1 - m, 7), (m, 9)], [(m, 11), (1 - m, 3), (m, 11)], [(m, int(plus[1])), (m, int(minus[1]))]]
        for sel in sels:
            out.append(dict(medium=m, users=[], penalties=pen, items=[dict(medium=a, matchedid=i) for a, i in sel]))
    return out


def test_literal_retrieval_is_the_vectorised_ordering():
    rng = np.random.default_rng(3)
    sim, which = ri.integer_tables(rng, V)
    released = {m: rng.random(V[m]) < 0.8 for m in (0, 1)}
    for st in _states(rng, which):
        m = st["medium"]
        for rel in (None, released[m]):
            lit, p = ri.retrieval_literal(m, sim, st, V, rel)
            ids, scores = ri.ordering_exact(m, sim, st, V, rel)
            assert np.array_equal(lit, ids)
            assert np.array_equal(p[lit], scores)
            assert ids.size == int(ri.admissible(m, st, V, rel).sum())
    empty = dict(medium=0, users=[], items=[])
    ids, scores = ri.ordering_exact(0, sim, empty, V)
    assert np.array_equal(ids, np.arange(1, V[0])) and not scores.any()          # no selection: ascending id, all +0.0
    zero = _states(rng, which)[4]
    assert not ri.prior_int(0, sim, zero, V).any()                              # v + (-v): the zero vector


def test_literal_render_is_the_windowed_oracle():
    rng = np.random.default_rng(4)
    sim, which = ri.integer_tables(rng, V)
    related = {f"{m}.related": rr.random_csc(rng, V[m], V[m], 0.05) for m in (0, 1)}
    pags = [dict(offset=0, limit=10), dict(offset=95, limit=7), dict(offset=290, limit=50), dict(offset=10 ** 6, limit=3)]
    for st in _states(rng, which)[::2]:
        m = st["medium"]
        ids, _ = ri.ordering_exact(m, sim, st, V)
        for pg in pags:
            page, total = ri.render_literal(st, pg, sim, related, V)
            assert total == ids.size
            win = ri.page_window(total, pg)
            if win is None:
                assert page.size == 0
                continue
            cand = ids[win[0]:win[1]]
            want = rk.reranking(st, cand, np.zeros(cand.size, np.float32), win[3], related[f"{m}.related"], sim[f"embeddings.{m}"].T)
            assert np.array_equal(page, want[win[2] - 1:win[3]])
        # the `/add_item` penalties: no reranking effect, the page is the ordering's slice
        plain = dict(st, penalties=dict(decay=0.9, mmr_penalty=0.0, same_series_penalty=0.0, related_penalty=0.0))
        page, _ = ri.render_literal(plain, dict(offset=20, limit=15), sim, related, V)
        assert np.array_equal(page, ids[20:35])


def test_window_from_exact_totals_is_serve_page_window():
    from recommendersystem_amd import serve
    rng = np.random.default_rng(5)
    for _ in range(2000):
        limit = int(rng.integers(1, 1025))
        total = int(rng.choice([0, 1, 1023, 1024, 1025, 8191, 8192, 8193, int(rng.integers(0, 200000))]))
        offset = int(rng.choice([0, total - 1 if total else 0, total, total + 5, int(rng.integers(0, max(total, 1) + 2000))]))
        pg = dict(offset=offset, limit=limit)
        assert ri.page_window(total, pg) == serve.page_window(total, pg)
        # the window rsys_render_items asks the retrieval for, before the total is known
        mitr = 1024 - 1024 % limit
        start = offset // mitr * mitr
        count = min(max(total - start, 0), mitr)
        win = serve.page_window(total, pg)
        if win is None:
            assert offset >= total
        else:
            assert (win[0], win[1] - win[0]) == (start, count) and 1 <= win[2] <= min(win[3], count)
            # (an offset that is no multiple of the limit can end the page past the ranked slice: win[3] > count, the page is cut there)


def test_render_items_rejects_states_with_users():
    from recommendersystem_amd import serve
    st = dict(medium=0, items=[], users=[dict(user=dict(items=[]))])
    with pytest.raises(ValueError, match="users"):
        serve.render_items(None, [st], dict(offset=0, limit=10))
    assert serve.render_items(None, [], dict(offset=0, limit=10)) == []


def test_python_argument_validation():
    import recommendersystem_amd as ra
    from recommendersystem_amd import serve
    bare = dict(medium=0, items=[], users=[])
    for pg in (dict(offset=-1, limit=10), dict(offset=0, limit=0), dict(offset=0, limit=1025)):
        with pytest.raises(ValueError):
            serve.render_items(None, [bare], pg)
        with pytest.raises(ValueError):
            serve.render(None, [dict(bare, users=[dict(user=dict(items=[]), embeds={})])], pg, exact=True)
    with pytest.raises(ValueError):
        serve.render_items(None, [dict(bare, medium=2)], dict(offset=0, limit=10))
    with pytest.raises(ValueError):
        serve.render_items(None, [bare, bare], [dict(offset=0, limit=10)])
    for win in ((-1, 10), (0, 0), (0, 1025)):
        with pytest.raises(ValueError):
            serve.retrieval_window(None, [bare], win)
    with pytest.raises(ValueError):
        serve.retrieval_window(None, [bare, bare], [(0, 10)])
    fake = types.SimpleNamespace(WINDOW_ROWS=1024, _h=None)
    call = ra.RecommenderModel.retrieve_window
    q = np.zeros((2, 4), np.float32)
    with pytest.raises(ValueError):
        call(fake, None, 0, [0, 0], [10])                                   # one length for two groups
    with pytest.raises(ValueError):
        call(fake, q, 0, [0, 0, 0], [1, 1, 1])                              # two queries, three groups, no group ids
    with pytest.raises(ValueError):
        call(fake, q, 0, [0], [1], group=[0])                               # one group id for two queries
    with pytest.raises(ValueError):
        call(fake, q, 0, [0, 0], [1, 1], histories=[[]])                    # one list for two queries
    with pytest.raises(ValueError):
        call(fake, None, 0, [0, 0], [1, 1], selected=[[]])                  # one selection for two groups
    with pytest.raises(ValueError):
        ra.RecommenderModel.render_items(fake, [0, 1], [0], [10, 10], np.zeros((2, 4)))
    with pytest.raises(ValueError):
        ra.RecommenderModel.render_items(fake, [0], [0], [10], np.zeros((1, 4)), selected=[[], []])
