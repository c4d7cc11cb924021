"""GPU: weighted multi-query states through whole requests (rsys_query_weights_set), at the sizes, tables and model
kinds of tests/test_gpu_render_request.py.  Expected values are float32 chains (tests/_query_weights_np.py) over the library's own
unweighted per-user terms, so every comparison is bit for bit."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _query_weights_np as qw  # noqa: E402
import _render_items_np as ri  # noqa: E402
import _render_rank_np as rk  # noqa: E402
import _render_retrieval_np as rr  # noqa: E402
import test_gpu_render_request as base  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = [("plain", "fp32"), ("plain", "bf16"), ("bank", "fp32"), ("bank", "bf16")]


def _with_embeds(model, states):
    """the "{m}.retrieval" embedding of every user, from the staged forward (what serve.retrieval / serve.render read)"""
    from recommendersystem_amd import serve
    for st in states:
        m = int(st["medium"])
        for u in st["users"]:
            u["embeds"] = {f"{m}.retrieval": serve.predict(model, [u["user"]], "retrieval", m)[0][f"{m}.retrieval"]}
    return states


def _weigh(states, user_w=None, item_w=None):
    """a deep copy with weights: a scalar for everyone, or flat lists in user / item order (None entries leave the key absent)"""
    out = copy.deepcopy(states)
    users = [u for st in out for u in st["users"]]
    items = [a for st in out for a in st["items"]]
    for entries, w in ((users, user_w), (items, item_w)):
        if w is None:
            continue
        ws = [w] * len(entries) if np.ndim(w) == 0 else list(w)
        assert len(ws) == len(entries)
        for e, x in zip(entries, ws):
            if x is not None:
                e["weight"] = float(x)
    return out


def _same_pages(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0]) and x[1] == y[1]


def _bare_states(V, seed=7):
    """states without users (render_items): both media, selected items of both media"""
    rng = np.random.default_rng(seed)
    states = []
    for m, ns in ((0, 2), (1, 3), (0, 1)):
        st = base._state(rng, V, m, 1, ns)
        st["users"] = []
        states.append(st)
    return states


# ---------------------------------------------------------------- 1. weights of one
@pytest.mark.parametrize("kind,dtype", KINDS)
def test_weights_of_one_change_nothing(kind, dtype):
    from recommendersystem_amd import serve
    cfg, model, V = base._model(kind, dtype)
    base._tables(model, V)
    states, pags, registry = base._request()
    _with_embeds(model, states)
    ones = _weigh(states, 1.0, 1.0)
    assert serve.state_weights(states) == (None, None) and all(w is not None for w in serve.state_weights(ones))
    # rsys_retrieve_request, rsys_retrieve_window, rsys_rank_request
    a, b = serve.retrieval(model, states, k=8192, coefs=[0.5]), serve.retrieval(model, ones, k=8192, coefs=[0.5])
    for (ia, sa), (ib, sb) in zip(a, b):
        assert np.array_equal(ia, ib) and sa.tobytes() == sb.tobytes()
    wins = [(3, 40)] * len(states)
    for (ia, sa, ta), (ib, sb, tb) in zip(serve.retrieval_window(model, states, wins), serve.retrieval_window(model, ones, wins)):
        assert np.array_equal(ia, ib) and sa.tobytes() == sb.tobytes() and ta == tb
    idxs = [x[0][:50] for x in a]
    for sts in (states, ones):
        for st, c in zip(sts, idxs):
            for u in st["users"]:
                u["embeds"][f"{st['medium']}.ranking"] = np.linspace(0, 9, c.size).astype(np.float32)
    for ra_, rb_ in zip(serve.ranking(model, states, idxs, registry), serve.ranking(model, ones, idxs, registry)):
        assert ra_.tobytes() == rb_.tobytes()
    # rsys_render_request / _full under every serving flag
    for flags in (dict(), dict(trim=True), dict(pack=True), dict(compact_top=True), dict(full_history=True),
                  dict(full_history=True, pack_ranking=True)):
        _same_pages(serve.render_users(model, states, pags, registry, **flags), serve.render_users(model, ones, pags, registry, **flags))
    # rsys_render_items
    bare = _bare_states(V)
    pg = {"offset": 4, "limit": 9}
    _same_pages(serve.render_items(model, bare, pg), serve.render_items(model, _weigh(bare, None, 1.0), pg))
    assert model.query_weights_pending() == (0, 0)
    model.close()


# ---------------------------------------------------------------- 2. - 4. the float32 chains on the library's own per-user terms
def _retrieval_case(dtype, seed=5):
    """a model with integer item-similarity tables, one state of 3 users and 2 selected items (one per medium), its request arrays"""
    from recommendersystem_amd import serve
    cfg, model, V = base._model("plain", dtype)
    rng = np.random.default_rng(seed)
    rel = rr.random_relations(rng, V, density=0.01)
    sim, _ = ri.integer_tables(rng, V)
    serve.load_retrieval_tables(model, rel, sim)
    m = 1
    st = base._state(rng, V, m, 3, 2)
    st["items"][0]["medium"], st["items"][1]["medium"] = m, 1 - m
    for a in st["items"]:
        a["matchedid"] = int(rng.integers(1, V[a["medium"]]))
    q = rng.standard_normal((3, cfg["embed_dim"])).astype(np.float32)
    hist = [[(int(x["medium"]), int(x["matchedid"]), int(x["status"])) for x in u["user"]["items"]] for u in st["users"]]
    sel = [[(int(a["medium"]), int(a["matchedid"])) for a in st["items"]]]
    return model, V, m, q, hist, sel


def _user_rows(model, q, m, Vm):
    """z - lse of every query over the whole medium: a one-query rsys_retrieve_topk with k = V returns exactly those bits"""
    rows = np.full((q.shape[0], Vm), np.nan, np.float32)
    for u in range(q.shape[0]):
        ids, scores, counts = model.retrieve_topk(q[u:u + 1], m, Vm)
        assert counts[0] == Vm
        rows[u, ids[0]] = scores[0]
    return rows


def _expected_retrieval(model, V, m, q, hist, sel, uw, sw):
    """(ids, scores) of the weighted request by the chain: the weighted prior of a user-less window, the users' rows, the masks of
    the unweighted request, then descending score with ties by ascending id"""
    Vm = V[m]
    rows = _user_rows(model, q, m, Vm)
    ids, scores, counts, totals = model.retrieve_window(None, m, [0], [1024], n_groups=1, selected=sel, selected_weights=sw)
    assert totals[0] == counts[0] < 1024
    prior = np.full(Vm, np.nan, np.float32)
    prior[ids[0, :counts[0]]] = scores[0, :counts[0]]
    ids0, _, c0 = model.retrieve_request(q, m, Vm, group=[0, 0, 0], histories=hist, selected=sel)
    adm = np.sort(ids0[0, :c0[0]])                                   # the unweighted request's masks
    s = qw.chain(prior[adm], rows[:, adm], uw) + np.float32(0.0)     # (-0.0 comes back as +0.0)
    ok = s > -np.inf
    adm, s = adm[ok], s[ok]
    order = np.lexsort((adm, -s.astype(np.float64)))
    return adm[order].astype(np.int32), s[order]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_retrieval_is_the_float32_chain(dtype):
    model, V, m, q, hist, sel = _retrieval_case(dtype)
    for uw, sw in (([0.5, -1.0, 2.25], [2.0, -0.5]), ([3e-3, 1.0, 0.5], None), (None, [-1.0, 0.25])):
        want_ids, want_s = _expected_retrieval(model, V, m, q, hist, sel, [1.0] * 3 if uw is None else uw, sw)
        ids, scores, counts = model.retrieve_request(q, m, V[m], group=[0, 0, 0], histories=hist, selected=sel, user_weights=uw,
                                                     selected_weights=sw)
        n = int(counts[0])
        assert n == want_ids.size and np.array_equal(ids[0, :n], want_ids)
        assert scores[0, :n].tobytes() == want_s.tobytes()
        # the same through the window call, at a window that starts inside the list
        wi, ws, wc, wt = model.retrieve_window(q, m, [7], [50], group=[0, 0, 0], n_groups=1, histories=hist, selected=sel, user_weights=uw,
                                               selected_weights=sw)
        assert wt[0] == n and np.array_equal(wi[0, :wc[0]], want_ids[7:57]) and ws[0, :wc[0]].tobytes() == want_s[7:57].tobytes()
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_zero_weight_user_in_retrieval(dtype):
    """a zero-weight user: the scores of the state without its terms, under the masks of the state with it"""
    model, V, m, q, hist, sel = _retrieval_case(dtype, seed=6)
    keep = [0, 2]
    ids_b, sc_b, c_b = model.retrieve_request(q[keep], m, V[m], group=[0, 0], histories=[hist[u] for u in keep], selected=sel)
    without = dict(zip(ids_b[0, :c_b[0]].tolist(), sc_b[0, :c_b[0]]))
    ids_a, _, c_a = model.retrieve_request(q, m, V[m], group=[0, 0, 0], histories=hist, selected=sel)
    for zero in (0.0, -0.0):
        ids, scores, counts = model.retrieve_request(q, m, V[m], group=[0, 0, 0], histories=hist, selected=sel, user_weights=[1.0, zero, 1.0])
        n = int(counts[0])
        assert n == c_a[0] and set(ids[0, :n].tolist()) == set(ids_a[0, :n].tolist())        # the masks of the state with the user
        assert np.array([without[i] for i in ids[0, :n].tolist()], np.float32).tobytes() == scores[0, :n].tobytes()
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ranking_is_the_float32_chain(dtype):
    cfg, model, V = base._model("plain", dtype)
    base._tables(model, V)
    rng = np.random.default_rng(8)
    m, nu, n = 1, 3, 150
    q = rng.standard_normal((nu, cfg["embed_dim"])).astype(np.float32)
    cand = [rng.choice(np.arange(1, V[m]), n, replace=False)]
    rm = [rng.uniform(0, 10, n).astype(np.float32) for _ in range(nu)]
    for coefs in (dict(), dict(retrieval_coef=0.5, rating_coefs=(0.3, 0.8), rating_mean=4.0)):
        rows = [model.rank_request(q[u:u + 1], m, cand, r_masked=[rm[u]], rerank=False, **coefs)[1][0] for u in range(nu)]
        plain = model.rank_request(q, m, cand, group=[0] * nu, r_masked=rm, rerank=False, **coefs)[1][0]
        for w in ([1.0, 1.0, 1.0], [0.5, -1.0, 2.25], [3e-3, 0.0, 1.0], [-0.0, 0.0, 0.0]):
            got = model.rank_request(q, m, cand, group=[0] * nu, r_masked=rm, rerank=False, user_weights=w, **coefs)[1][0]
            assert got.tobytes() == qw.chain(np.zeros(n, np.float32), rows, w).tobytes(), w
            if w == [1.0, 1.0, 1.0]:
                assert got.tobytes() == plain.tobytes()
        # the zero-weight user: the two others alone
        two = model.rank_request(q[[0, 2]], m, cand, group=[0, 0], r_masked=[rm[0], rm[2]], rerank=False, **coefs)[1][0]
        got = model.rank_request(q, m, cand, group=[0] * nu, r_masked=rm, rerank=False, user_weights=[1.0, 0.0, 1.0], **coefs)[1][0]
        assert got.tobytes() == two.tobytes()
    model.close()


# ---------------------------------------------------------------- 5. the one-call pipelines against the staged path
def _mixed_weights(states):
    """every user and item weighted: one zero user weight, one negative item weight, the rest mixed"""
    nu = sum(len(st["users"]) for st in states)
    ni = sum(len(st["items"]) for st in states)
    uw = [[0.5, 2.25, 1.0, -1.0, 3e-3, 1.5][i % 6] for i in range(nu)]
    uw[4] = 0.0
    iw = [[2.0, 0.5, 1.0][i % 3] for i in range(ni)]
    iw[1] = -0.75
    return _weigh(states, uw, iw)


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_pipelines_against_the_staged_path(kind, dtype):
    from recommendersystem_amd import serve
    cfg, model, V = base._model(kind, dtype)
    base._tables(model, V)
    states, pags, registry = base._request()
    assert len(states) == 5 and sum(len(st["users"]) for st in states) == 9
    ws = _mixed_weights(_with_embeds(model, states))
    model.render_keep(True)
    out = serve.render_users(model, ws, pags, registry)
    rm_users = model.render_kept("rm_users").reshape(-1, 3)
    r_masked = model.render_kept("r_masked")
    model.render_keep(False)
    staged = serve.render(model, ws, pags, registry)                  # (leaves each user's "{m}.ranking" in its embeds)
    _same_pages(out, staged)
    assert any(o[0].size for o in out)
    plain = serve.render_users(model, states, pags, registry)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(out, plain))          # (the weights do reach the pages)
    users = [(st, u) for st in ws for u in st["users"]]
    for ui, o, n in rm_users:
        st, u = users[ui]
        base._close(r_masked[o:o + n], u["embeds"][f"{st['medium']}.ranking"], dtype, "ranking", f"kept r_masked vs the staged path (user {ui})")
    _same_pages(serve.render_users(model, ws, pags, registry, full_history=True), serve.render(model, ws, pags, registry, full_history=True))
    # a deep offset: the staged path on the windowed retrieval (exact=True) and the one-call pipeline give the same page
    deep = [{"offset": 60, "limit": 7}] * len(ws)
    a = serve.render(model, ws, deep, registry, exact=True)
    _same_pages(a, serve.render_users(model, ws, deep, registry))
    assert any(o[0].size for o in a)
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_render_items_with_weighted_items(dtype):
    """rsys_render_items on integer tables with dyadic weights (every product and sum exact): the ordering from the weighted prior in
    float64, the page window, the reranking of tests/_render_rank_np.py on zeros"""
    from recommendersystem_amd import serve
    cfg, model, V = base._model("plain", dtype)
    rng = np.random.default_rng(12)
    sim, _ = ri.integer_tables(rng, V)
    related = {f"{m}.related": rr.random_csc(rng, V[m], V[m], 0.05) for m in (0, 1)}
    serve.load_retrieval_tables(model, rr.random_relations(rng, V, density=0.01), sim)
    serve.load_ranking_tables(model, related)
    bare = _weigh(_bare_states(V), None, [2.0, -0.5, 1.0, 0.25, -1.0, 0.0])
    pags = [{"offset": 0, "limit": 10}, {"offset": 23, "limit": 7}, {"offset": 5, "limit": 5}]
    got = serve.render_items(model, bare, pags)
    plain = serve.render_items(model, _bare_states(V), pags)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(got, plain))
    for st, pg, (page, total) in zip(bare, pags, got):
        m = int(st["medium"])
        Em = sim[f"embeddings.{m}"].astype(np.float64)
        s = np.zeros(Em.shape[0])
        for a in st["items"]:
            x = sim[f"embeddings.{a['medium']}"].astype(np.float64)[:, a["matchedid"]]
            s += a["weight"] * (x if a["medium"] == m else sim[f"crossproject.{a['medium']}"].astype(np.float64) @ x)
        p = Em.T @ s
        ids = np.flatnonzero(ri.admissible(m, st, V))
        ids = ids[np.lexsort((ids, -p[ids]))]
        assert total == ids.size
        start, stop, sidx, eidx = ri.page_window(total, pg)
        picks = rk.reranking(st, ids[start:stop], np.zeros(stop - start, np.float32), eidx, related[f"{m}.related"],
                             sim[f"embeddings.{m}"].T)
        assert np.array_equal(page, np.asarray(picks[sidx - 1:eidx], np.int32))
    model.close()


# ---------------------------------------------------------------- 6. the one-shot setter
def test_setter_is_one_shot_and_checks_counts():
    import recommendersystem_amd as ra
    from recommendersystem_amd._lib import lib
    model, V, m, q, hist, sel = _retrieval_case("fp32")
    L, Vm = lib(), V[m]
    kw = dict(group=[0, 0, 0], histories=hist, selected=sel)
    plain = model.retrieve_request(q, m, Vm, **kw)
    weighted = model.retrieve_request(q, m, Vm, user_weights=[0.5, -1.0, 2.25], selected_weights=[2.0, -0.5], **kw)
    assert not np.array_equal(weighted[0], plain[0])
    again = model.retrieve_request(q, m, Vm, **kw)                    # a second request without setting again: unweighted
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, plain))
    # a weighted request run twice gives equal bits
    twice = model.retrieve_request(q, m, Vm, user_weights=[0.5, -1.0, 2.25], selected_weights=[2.0, -0.5], **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(twice, weighted))
    # pending, replaced, cleared
    model.set_query_weights([1, 2, 3], [4, 5])
    assert model.query_weights_pending() == (3, 2)
    model.set_query_weights(None, [4, 5])
    assert model.query_weights_pending() == (0, 2)
    model.retrieve_topk(q, m, 5)                                      # not a consumer
    assert model.query_weights_pending() == (0, 2)
    model.set_query_weights(None, None)
    assert model.query_weights_pending() == (0, 0)
    # a NaN weight: refused, nothing held (what was held is dropped too)
    model.set_query_weights([1, 2, 3], None)
    bad = np.array([1.0, np.nan, 2.0], np.float32)
    assert L.rsys_query_weights_set(model._h, bad.ctypes.data, 3, None, 0) == -1
    assert model.query_weights_pending() == (0, 0)
    inf = np.array([np.inf], np.float32)
    assert L.rsys_query_weights_set(model._h, None, 0, inf.ctypes.data, 1) == -1
    # wrong counts: RSYS_ERR_ARG, outputs untouched, nothing left pending
    gp = np.zeros(3, np.int32)
    from recommendersystem_amd.model import triples_csr
    h, s = triples_csr(hist, 3), triples_csr(sel, 2)
    for uw, sw in (([1.0, 2.0], None), (None, [1.0]), ([1.0] * 4, [1.0, 1.0])):
        model.set_query_weights(uw, sw)
        ids = np.full((1, Vm), -7, np.int32); scores = np.full((1, Vm), -7, np.float32); counts = np.full(1, -7, np.int32)
        rc = L.rsys_retrieve_request(model._h, m, q.ctypes.data, 3, gp.ctypes.data, 1, *[a.ctypes.data for a in h], *[a.ctypes.data for a in s],
                                     Vm, ids.ctypes.data, scores.ctypes.data, counts.ctypes.data)
        assert rc == -1 and (ids == -7).all() and (scores == -7).all() and (counts == -7).all()
        assert model.query_weights_pending() == (0, 0)
    # selected-item weights before rsys_rank_request, user weights before rsys_render_items: ARG errors that consume them
    base._tables(model, V)
    cand = [np.arange(1, 20)]
    model.set_query_weights(None, [1.0, 2.0])
    with pytest.raises(ra.RsysError):
        model.rank_request(q, m, cand, group=[0, 0, 0], r_masked=[np.zeros(19, np.float32)] * 3, rerank=False)
    assert model.query_weights_pending() == (0, 0)
    model.set_query_weights([1.0], None)
    with pytest.raises(ra.RsysError):
        model.render_items([m], [0], [5], np.zeros((1, 4), np.float32), sel)
    assert model.query_weights_pending() == (0, 0)
    # given scores: no weights are read, but they are consumed
    model.set_query_weights([9.0, 9.0, 9.0], None)
    model.rank_request(None, m, cand, group=[0, 0, 0], partialk=[5], penalties=np.zeros((1, 4), np.float32), scores=[np.arange(19, dtype=np.float32)])
    assert model.query_weights_pending() == (0, 0)
    model.close()


# ---------------------------------------------------------------- 7. a weighted request between training steps
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_request_between_training_steps_changes_nothing(dtype):
    """Deterministic mode: step -> load tables + weighted render_users -> step gives the step -> step results bit for bit."""
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import serve
    cfg = synth.make_config("hd64", mask_rate=0.2, deterministic=True)
    V = (cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"])
    P = synth.make_params(cfg, 3, "test")
    rows = 4
    batches = [synth.make_batch(cfg, rows, 40 + i) for i in range(2)]
    masks = [synth.make_masks(cfg, rows, 50 + i) for i in range(2)]
    names = synth.trainable_names(cfg)
    states, pags, registry = base._request(seed=44)
    ws = _mixed_weights(states)

    def run(with_request):
        model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
        model.load_state_dict(P)
        opt = ra.create_optimizer(model, dict(cfg, learning_rate=1e-2))
        model.set_loss_weights(base.TASK_W, 1)
        out, pages = [], None
        for i, (d, mk) in enumerate(zip(batches, masks)):
            if i == 1 and with_request:
                base._tables(model, V)
                pages = serve.render_users(model, ws, pags, registry)
                _same_pages(pages, serve.render_users(model, ws, pags, registry))       # run twice: equal bits
            out.append(np.array(model(d, False, masks=mk), np.float32))
            out += [model.grad(n).copy() for n in names]
            opt.step(clip_max_norm=1.0)
        out += [model.get_parameter(n).copy() for n in names]
        model.close()
        return out

    a, b = run(False), run(True)
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
