"""GPU: text queries in request states (rsys_query_texts_set), at the sizes, tables and model kinds of
tests/test_gpu_render_request.py and by the method of tests/test_gpu_query_weights.py: expected values are float32 chains
(tests/_query_texts_np.py) over the library's own per-text rows (rsys_op_text_rows) and per-user terms, so every comparison is bit for
bit."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _query_texts_np as qt  # noqa: E402
import test_gpu_query_weights as wq  # noqa: E402
import test_gpu_render_request as base  # noqa: E402

pytestmark = pytest.mark.gpu

Q = 64
KINDS = [("plain", "fp32"), ("plain", "bf16"), ("bank", "fp32"), ("bank", "bf16")]
TEXT_W = ([1.0, 0.5], [-1.0, 0.0], [-0.0, 0.5], [0.5, -1.0], None)      # weights from {1, 0.5, -1, +0.0, -0.0}; None = 1.0 each


def _search(model, cfg, V, dtype, seed=3):
    """one search handle per medium on the model's item table, with a random encoder"""
    from recommendersystem_amd import search
    rng = np.random.default_rng(seed)
    out = {}
    for m in (0, 1):
        scfg = search.training_config({m: V[m]}, batch_size=64, embed_dim=cfg["embed_dim"], query_dim=Q)
        s = search.SearchModel(scfg, m, model, dtype=dtype, max_batch=64)
        s.param_set("encoder.weight", (rng.standard_normal((Q, cfg["embed_dim"])) * 1.5 / np.sqrt(Q)).astype(np.float32))
        s.param_set("logit_scale", 1.0)
        out[m] = s
    return out


def _emb(rng, n):
    return rng.standard_normal((n, Q)).astype(np.float32)


def _with_texts(states, rng, weights=None, per_state=(2, 1, 0, 1, 2)):
    """a deep copy with text queries: per_state[j] texts in state j; weights: a scalar for every text, a flat list, or None (no key)"""
    out = copy.deepcopy(states)
    k = 0
    for st, n in zip(out, per_state):
        if n == 0:
            continue
        st["texts"] = []
        for e in _emb(rng, n):
            t = {"embedding": e}
            if weights is not None:
                t["weight"] = float(weights if np.ndim(weights) == 0 else weights[k])
            st["texts"].append(t)
            k += 1
    return out


def _order(adm, s):
    s = s + np.float32(0.0)                                          # (-0.0 comes back as +0.0)
    ok = s > -np.inf
    adm, s = adm[ok], s[ok]
    o = np.lexsort((adm, -s.astype(np.float64)))
    return adm[o].astype(np.int32), s[o]


# ---------------------------------------------------------------- 1. retrieval: prior, then texts, then users
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_retrieval_is_the_float32_chain(dtype):
    model, V, m, q, hist, sel = wq._retrieval_case(dtype)
    S = _search(model, model.config, V, dtype)
    Vm = V[m]
    x = _emb(np.random.default_rng(11), 2)
    z, lse = S[m].text_rows(x)
    rows = wq._user_rows(model, q, m, Vm)
    ids, scores, counts, totals = model.retrieve_window(None, m, [0], [1024], n_groups=1, selected=sel)
    prior = np.full(Vm, np.nan, np.float32)
    prior[ids[0, :counts[0]]] = scores[0, :counts[0]]
    kw = dict(group=[0, 0, 0], histories=hist, selected=sel)
    ids0, sc0, c0 = model.retrieve_request(q, m, Vm, **kw)
    adm = np.sort(ids0[0, :c0[0]])                                   # texts carry no masks: those of the request without them
    for tw in TEXT_W:
        for uw in (None, [0.5, -1.0, 2.25]):
            want_ids, want_s = _order(adm, qt.retrieval(prior[adm], z[:, adm], lse, tw, rows[:, adm], uw))
            model.query_texts_set(S[m], m, x, [0, 0], tw)
            assert model.query_texts_pending() == ((2, 0) if m == 0 else (0, 2))
            got_i, got_s, got_c = model.retrieve_request(q, m, Vm, user_weights=uw, **kw)
            assert model.query_texts_pending() == (0, 0)
            n = int(got_c[0])
            assert n == want_ids.size and np.array_equal(got_i[0, :n], want_ids), (tw, uw)
            assert got_s[0, :n].tobytes() == want_s.tobytes(), (tw, uw)
            # the window call, at a window that starts inside the list
            model.query_texts_set(S[m], m, x, [0, 0], tw)
            wi, ws, wc, wt = model.retrieve_window(q, m, [7], [50], n_groups=1, user_weights=uw, **kw)
            assert wt[0] == n and np.array_equal(wi[0, :wc[0]], want_ids[7:57]) and ws[0, :wc[0]].tobytes() == want_s[7:57].tobytes()
    # a zero-weight text leaves every bit of the request without it; two zero weights every bit of the request without texts
    model.query_texts_set(S[m], m, x[:1], [0], [0.5])
    one = model.retrieve_request(q, m, Vm, **kw)
    for zero in (0.0, -0.0):
        model.query_texts_set(S[m], m, x, [0, 0], [0.5, zero])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(model.retrieve_request(q, m, Vm, **kw), one))
        model.query_texts_set(S[m], m, x, [0, 0], [zero, zero])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(model.retrieve_request(q, m, Vm, **kw), (ids0, sc0, c0)))
    assert not np.array_equal(one[0], ids0)                          # (the text does reach the order)
    for s in S.values():
        s.close()
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_window_groups_with_texts_only(dtype):
    """groups without users: prior + texts, and texts alone (no selected item: the zero fill); a group without texts beside them"""
    model, V, m, q, hist, sel = wq._retrieval_case(dtype)
    S = _search(model, model.config, V, dtype)
    Vm = V[m]
    x = _emb(np.random.default_rng(12), 3)
    z, lse = S[m].text_rows(x)
    sel3 = [sel[0], [], sel[0]]
    ids, scores, counts, totals = model.retrieve_window(None, m, [0] * 3, [1024] * 3, n_groups=3, selected=sel3)
    assert (totals == counts).all() and (counts < 1024).all()
    tg = [1, 0, 1]                                                    # text -> group: group 1 (no selected item) holds texts 0 and 2
    for tw in ([1.0, 0.5, -1.0], [0.0, 1.0, -0.0], None):
        model.query_texts_set(S[m], m, x, tg, tw)
        gi, gs, gc, gt = model.retrieve_window(None, m, [0] * 3, [1024] * 3, n_groups=3, selected=sel3)
        assert model.query_texts_pending() == (0, 0)
        for g in range(3):
            adm = np.sort(ids[g, :counts[g]])
            prior = np.full(Vm, np.nan, np.float32)
            prior[ids[g, :counts[g]]] = scores[g, :counts[g]]
            mine = [t for t in range(3) if tg[t] == g]
            want_ids, want_s = _order(adm, qt.userless(prior[adm], z[mine][:, adm], lse[mine], None if tw is None else [tw[t] for t in mine]))
            assert gt[g] == gc[g] == want_ids.size and np.array_equal(gi[g, :gc[g]], want_ids), (tw, g)
            assert gs[g, :gc[g]].tobytes() == want_s.tobytes(), (tw, g)
    for s in S.values():
        s.close()
    model.close()


# ---------------------------------------------------------------- 2. ranking: +0.0, then texts, then users
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ranking_is_the_float32_chain(dtype):
    cfg, model, V = base._model("plain", dtype)
    base._tables(model, V)
    S = _search(model, cfg, V, dtype)
    rng = np.random.default_rng(8)
    m, nu, n = 1, 2, 150
    q = rng.standard_normal((nu, cfg["embed_dim"])).astype(np.float32)
    cand = [rng.choice(np.arange(1, V[m]), n, replace=False)]
    rm = [rng.uniform(0, 10, n).astype(np.float32) for _ in range(nu)]
    x = _emb(rng, 2)
    z, lse = S[m].text_rows(x)
    for coefs in (dict(), dict(retrieval_coef=0.5, rating_coefs=(0.3, 0.8), rating_mean=4.0)):
        rows = [model.rank_request(q[u:u + 1], m, cand, r_masked=[rm[u]], rerank=False, **coefs)[1][0] for u in range(nu)]
        plain = model.rank_request(q, m, cand, group=[0] * nu, r_masked=rm, rerank=False, **coefs)[1][0]
        for tw in TEXT_W:
            for uw in (None, [0.5, -1.0]):
                model.query_texts_set(S[m], m, x, [0, 0], tw)
                got = model.rank_request(q, m, cand, group=[0] * nu, r_masked=rm, rerank=False, user_weights=uw, **coefs)[1][0]
                assert model.query_texts_pending() == (0, 0)
                assert got.tobytes() == qt.ranking(z, lse, cand[0], tw, rows, uw).tobytes(), (tw, uw)
        for zero in (0.0, -0.0):
            model.query_texts_set(S[m], m, x, [0, 0], [zero, zero])
            assert model.rank_request(q, m, cand, group=[0] * nu, r_masked=rm, rerank=False, **coefs)[1][0].tobytes() == plain.tobytes()
    # given scores: the texts are consumed and not read
    kw = dict(group=[0] * nu, partialk=[5], penalties=np.zeros((1, 4), np.float32), scores=[np.arange(n, dtype=np.float32)])
    want = model.rank_request(None, m, cand, **kw)[0][0]
    model.query_texts_set(S[m], m, x, [0, 0], [9.0, 9.0])
    assert np.array_equal(model.rank_request(None, m, cand, **kw)[0][0], want) and model.query_texts_pending() == (0, 0)
    for s in S.values():
        s.close()
    model.close()


# ---------------------------------------------------------------- 3. the six entry points without texts, and with texts of weight zero
@pytest.mark.parametrize("kind,dtype", KINDS)
def test_no_texts_and_zero_weight_texts_change_nothing(kind, dtype):
    from recommendersystem_amd import serve
    cfg, model, V = base._model(kind, dtype)
    base._tables(model, V)
    S = _search(model, cfg, V, dtype)
    states, pags, registry = base._request()
    wq._with_embeds(model, states)
    zeros = _with_texts(states, np.random.default_rng(20), weights=[0.0, -0.0, 0.0, -0.0, 0.0, 0.0])
    assert serve.state_texts(states) is None and serve.state_texts(zeros)[0].shape == (6, Q)
    calls = []
    setter = model.query_texts_set
    model.query_texts_set = lambda *a, **k: (calls.append(a[1]), setter(*a, **k))[1]
    # rsys_retrieve_request, rsys_retrieve_window, rsys_rank_request
    a = serve.retrieval(model, states, k=8192, coefs=[0.5])
    assert calls == []                                               # states without a "texts" key never reach the setter
    b = serve.retrieval(model, zeros, k=8192, coefs=[0.5], search=S)
    assert sorted(calls) == [0, 1]
    for (ia, sa), (ib, sb) in zip(a, b):
        assert np.array_equal(ia, ib) and sa.tobytes() == sb.tobytes()
    wins = [(3, 40)] * len(states)
    for (ia, sa, ta), (ib, sb, tb) in zip(serve.retrieval_window(model, states, wins, search=S), serve.retrieval_window(model, zeros, wins, search=S)):
        assert np.array_equal(ia, ib) and sa.tobytes() == sb.tobytes() and ta == tb
    idxs = [x[0][:50] for x in a]
    for sts in (states, zeros):
        for st, c in zip(sts, idxs):
            for u in st["users"]:
                u["embeds"][f"{st['medium']}.ranking"] = np.linspace(0, 9, c.size).astype(np.float32)
    for ra_, rb_ in zip(serve.ranking(model, states, idxs, registry), serve.ranking(model, zeros, idxs, registry, search=S)):
        assert ra_.tobytes() == rb_.tobytes()
    # rsys_render_request / _full under every serving flag
    for flags in (dict(), dict(trim=True), dict(pack=True), dict(compact_top=True), dict(full_history=True),
                  dict(full_history=True, pack_ranking=True)):
        n = len(calls)
        plain = serve.render_users(model, states, pags, registry, search=S, **flags)
        assert len(calls) == n
        wq._same_pages(plain, serve.render_users(model, zeros, pags, registry, search=S, **flags))
    # rsys_render_items
    bare = wq._bare_states(V)
    pg = {"offset": 4, "limit": 9}
    wq._same_pages(serve.render_items(model, bare, pg), serve.render_items(model, _with_texts(bare, np.random.default_rng(21), 0.0, (1, 2, 0)), pg, search=S))
    assert model.query_texts_pending() == (0, 0)
    # texts without a matching `search` entry raise, before any request runs
    with pytest.raises(ValueError):
        serve.retrieval(model, zeros, k=8192, search={0: S[0]})
    with pytest.raises(ValueError):                                  # mixed media in one call: medium 0's set is not made either
        serve.render_users(model, zeros, pags, registry, search={0: S[0]})
    assert model.query_texts_pending() == (0, 0)
    # the request's Python wrapper raises after the sets were made: they are cleared, not left for the next request
    real = model.render_items
    model.render_items = lambda *a, **k: (_ for _ in ()).throw(ValueError("a check of the wrapper"))
    with pytest.raises(ValueError):
        serve.render_items(model, _with_texts(bare, np.random.default_rng(21), 0.0, (1, 2, 0)), pg, search=S)
    model.render_items = real
    assert model.query_texts_pending() == (0, 0)
    for s in S.values():
        s.close()
    model.close()


# ---------------------------------------------------------------- 4. the one-call pipelines against the staged path
@pytest.mark.parametrize("kind,dtype", KINDS)
def test_pipelines_against_the_staged_path(kind, dtype):
    from recommendersystem_amd import serve
    cfg, model, V = base._model(kind, dtype)
    base._tables(model, V)
    S = _search(model, cfg, V, dtype)
    states, pags, registry = base._request()
    assert [st["medium"] for st in states] == [1, 0, 1, 0, 1]
    wq._with_embeds(model, states)
    ts = _with_texts(states, np.random.default_rng(22), weights=[1.0, 0.5, -1.0, 2.0, 0.0, 1.5])     # texts in states of both media
    ts[1]["users"][0]["weight"] = 0.5                                # (with a weighted user and a weighted selected item beside them)
    ts[4]["items"][1]["weight"] = -0.75
    out = serve.render_users(model, ts, pags, registry, search=S)
    assert model.query_texts_pending() == (0, 0)
    wq._same_pages(out, serve.render(model, ts, pags, registry, search=S))
    assert any(o[0].size for o in out)
    no_texts = [{k: v for k, v in st.items() if k != "texts"} for st in ts]
    plain = serve.render_users(model, no_texts, pags, registry)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(out, plain))          # (the texts do reach the pages)
    wq._same_pages(serve.render_users(model, ts, pags, registry, full_history=True, search=S),
                   serve.render(model, ts, pags, registry, full_history=True, search=S))
    deep = [{"offset": 60, "limit": 7}] * len(ts)
    a = serve.render(model, ts, deep, registry, exact=True, search=S)
    wq._same_pages(a, serve.render_users(model, ts, deep, registry, search=S))
    assert any(o[0].size for o in a)
    # the serving flags with texts: the staged path under the same flag where it has one, and the texts reach the pages under each
    for flags in (dict(trim=True), dict(compact_top=True)):
        wq._same_pages(serve.render_users(model, ts, pags, registry, search=S, **flags), serve.render(model, ts, pags, registry, search=S, **flags))
    # packing changes which forwards run, not the pages: the packed calls against the same request unpacked
    wq._same_pages(serve.render_users(model, ts, pags, registry, search=S, pack=True), out)
    wq._same_pages(serve.render_users(model, ts, pags, registry, search=S, full_history=True, pack_ranking=True),
                   serve.render_users(model, ts, pags, registry, search=S, full_history=True))
    for flags in (dict(trim=True), dict(pack=True), dict(compact_top=True), dict(full_history=True), dict(full_history=True, pack_ranking=True)):
        with_t = serve.render_users(model, ts, pags, registry, search=S, **flags)
        without = serve.render_users(model, no_texts, pags, registry, **flags)
        assert any(not np.array_equal(a[0], b[0]) for a, b in zip(with_t, without)), flags
        assert [o[1] for o in with_t] == [o[1] for o in without]     # texts carry no masks: the totals stay
    for s in S.values():
        s.close()
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_render_items_against_the_staged_path(dtype):
    """rsys_render_items with texts: the window of `retrieval_window` on prior + texts, then `reranking` on zeros (r = +0.0: the texts do
    not enter the ranking scores of a state without users)"""
    from recommendersystem_amd import serve
    cfg, model, V = base._model("plain", dtype)
    base._tables(model, V)
    S = _search(model, cfg, V, dtype)
    bare = _with_texts(wq._bare_states(V), np.random.default_rng(23), weights=[1.0, -0.5, 2.0], per_state=(1, 2, 0))
    bare.append(dict(wq._bare_states(V, seed=9)[1], items=[], texts=[{"embedding": _emb(np.random.default_rng(24), 1)[0]}]))   # a phrase alone
    pags = [{"offset": 0, "limit": 10}, {"offset": 23, "limit": 7}, {"offset": 5, "limit": 5}, {"offset": 0, "limit": 12}]
    got = serve.render_items(model, bare, pags, search=S)
    assert model.query_texts_pending() == (0, 0)
    plain = serve.render_items(model, [{k: v for k, v in st.items() if k != "texts"} for st in bare], pags)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(got, plain))
    for st, pg, (page, total) in zip(bare, pags, got):
        mitr = 1024 - 1024 % pg["limit"]
        ids, _, tot = serve.retrieval_window(model, [st], [(pg["offset"] // mitr * mitr, mitr)], search=S)[0]
        assert tot == total
        start, stop, sidx, eidx = serve.page_window(tot, pg)
        stand_in = dict(st, users=[{"user": {"items": []}}])          # one user without a list stands in for the absent users
        picks = serve.reranking(model, [stand_in], [ids], [np.zeros(ids.size, np.float32)], eidx)[0]
        assert np.array_equal(page, picks[sidx - 1:eidx])
    for s in S.values():
        s.close()
    model.close()


# ---------------------------------------------------------------- 5. the one-shot setter
def test_setter_is_one_shot_and_checks_its_arguments():
    import ctypes as C

    import recommendersystem_amd as ra
    from recommendersystem_amd._lib import lib
    from recommendersystem_amd.model import triples_csr
    model, V, m, q, hist, sel = wq._retrieval_case("fp32")
    S = _search(model, model.config, V, "fp32")
    L, Vm, o = lib(), V[m], 1 - m
    pend = lambda a, b: (a, b) if m == 0 else (b, a)                  # (texts of medium m, of the other medium)
    x = _emb(np.random.default_rng(30), 3)
    kw = dict(group=[0, 0, 0], histories=hist, selected=sel)
    plain = model.retrieve_request(q, m, Vm, **kw)
    model.query_texts_set(S[m], m, x, [0, 0, 0], [1.0, 0.5, -1.0])
    first = model.retrieve_request(q, m, Vm, **kw)
    assert not np.array_equal(first[0], plain[0])
    again = model.retrieve_request(q, m, Vm, **kw)                    # a second request without setting again: no texts
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, plain))
    model.query_texts_set(S[m], m, x, [0, 0, 0], [1.0, 0.5, -1.0])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(model.retrieve_request(q, m, Vm, **kw), first))     # equal bits from call to call
    # pending per medium, replaced, cleared; rsys_retrieve_topk and the search entry points are no consumers
    model.query_texts_set(S[m], m, x, [0, 0, 0])
    model.query_texts_set(S[o], o, x[:2], [0, 0])
    assert model.query_texts_pending() == pend(3, 2)
    model.query_texts_set(S[m], m, x[:1], [0])
    assert model.query_texts_pending() == pend(1, 2)
    model.retrieve_topk(q, m, 5)
    S[m].topk(x, 3)
    S[m].text_rows(x)
    assert model.query_texts_pending() == pend(1, 2)
    model.query_texts_set(S[o], o, x[:0], [])
    assert model.query_texts_pending() == pend(1, 0)
    # refused sets: RSYS_ERR_ARG and nothing held for that medium (what was held is dropped); a bad medium changes nothing
    g3 = np.zeros(3, np.int32)
    bad_x = x.copy(); bad_x[1, 7] = np.nan
    bad_w = np.array([1.0, np.inf, 1.0], np.float32)
    big = np.zeros((65, Q), np.float32); g65 = np.zeros(65, np.int32)
    assert L.rsys_query_texts_set(model._h, S[m].h, 2, x.ctypes.data, 3, g3.ctypes.data, None) == -1
    assert model.query_texts_pending() == pend(1, 0)
    for args in ((None, x.ctypes.data, 3, g3.ctypes.data, None),                  # a null handle
                 (S[o].h, x.ctypes.data, 3, g3.ctypes.data, None),               # a handle whose V_m is the other medium's
                 (S[m].h, bad_x.ctypes.data, 3, g3.ctypes.data, None),
                 (S[m].h, x.ctypes.data, 3, g3.ctypes.data, bad_w.ctypes.data),
                 (S[m].h, x.ctypes.data, 3, None, None),
                 (S[m].h, big.ctypes.data, 65, g65.ctypes.data, None)):
        model.query_texts_set(S[m], m, x[:1], [0])
        assert L.rsys_query_texts_set(model._h, args[0], m, *args[1:]) == -1
        assert model.query_texts_pending() == (0, 0)
    hnd = C.c_void_p()
    assert L.rsys_search_create(Vm, model.config["embed_dim"], Q, 0, 8, 0, C.byref(hnd)) == 0          # features never set
    assert L.rsys_query_texts_set(model._h, hnd, m, x.ctypes.data, 3, g3.ctypes.data, None) == -1
    L.rsys_search_destroy(hnd)
    # consumed on error; a wrong-medium set and an out-of-range group: RSYS_ERR_ARG with outputs untouched
    gp = np.zeros(3, np.int32)
    h, s = triples_csr(hist, 3), triples_csr(sel, 2)

    def raw_request(k=Vm):
        ids = np.full((1, Vm), -7, np.int32); scores = np.full((1, Vm), -7, np.float32); counts = np.full(1, -7, np.int32)
        rc = L.rsys_retrieve_request(model._h, m, q.ctypes.data, 3, gp.ctypes.data, 1, *[a.ctypes.data for a in h], *[a.ctypes.data for a in s],
                                     k, ids.ctypes.data, scores.ctypes.data, counts.ctypes.data)
        return rc, bool((ids == -7).all() and (scores == -7).all() and (counts == -7).all())

    model.query_texts_set(S[m], m, x, [0, 0, 0])
    assert raw_request(k=0) == (-1, True) and model.query_texts_pending() == (0, 0)      # the call's own error: consumed all the same
    model.query_texts_set(S[o], o, x[:2], [0, 0])
    assert raw_request() == (-1, True) and model.query_texts_pending() == (0, 0)
    model.query_texts_set(S[m], m, x[:2], [0, 1])
    assert raw_request() == (-1, True) and model.query_texts_pending() == (0, 0)
    model.query_texts_set(S[m], m, x[:2], [0, -1])
    assert raw_request() == (-1, True) and model.query_texts_pending() == (0, 0)
    assert raw_request()[0] == 0
    # the pipelines check the group's medium
    base._tables(model, V)
    model.query_texts_set(S[o], o, x[:1], [0])
    with pytest.raises(ra.RsysError):
        model.render_items([m], [0], [5], np.zeros((1, 4), np.float32), sel)
    assert model.query_texts_pending() == (0, 0)
    model.query_texts_set(S[m], m, x[:1], [0])
    pages, totals = model.render_items([m], [0], [5], np.zeros((1, 4), np.float32), sel)
    assert model.query_texts_pending() == (0, 0) and pages[0].size == 5
    for sm in S.values():
        sm.close()
    model.close()
