"""GPU: a page for states without users in one device call (rsys_render_items) and serve.render(..., exact=True).
The retrieval stage is pinned exactly by an int64 oracle on integer-valued tables (tests/_render_items_np.py); the reranking stage
by the existing rsys_rank_request on the oracle's window with zero scores and one dummy user; plus side effects and reproducibility."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_items_np as ri  # noqa: E402
import _render_retrieval_np as rr  # noqa: E402

pytestmark = pytest.mark.gpu

BIG = (9500, 2000)
TASK_W = [0.05, 0.2, 0.3, 0.25]
PEN = dict(decay=0.9, mmr_penalty=0.25, same_series_penalty=0.5, related_penalty=0.5)


def _cfg(vocab=None, **kw):
    from oracle import synth
    cfg = synth.make_config("hd64", mask_rate=0.2, mask_topk=4, **kw)
    if vocab:
        cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"] = vocab
    return cfg


def _integer_model(dtype="fp32"):
    """hd64 model with V = (9500, 2000), the integer similarity tables, a random `related` table and a released mask; no relation tables"""
    import recommendersystem_amd as ra
    from recommendersystem_amd import serve
    model = ra.RecommenderModel(_cfg(BIG), dtype=dtype, max_rows=4)
    model.init_weights(9)
    model.random_pretrained_embeddings(10)
    rng = np.random.default_rng(41)
    sim, which = ri.integer_tables(rng, BIG)
    related = {f"{m}.related": rr.random_csc(rng, BIG[m], BIG[m], 4.0 / BIG[m]) for m in (0, 1)}
    released = {m: rng.random(BIG[m]) < 0.9 for m in (0, 1)}
    serve.load_retrieval_tables(model, {}, sim, released)
    serve.load_ranking_tables(model, related)
    return dict(model=model, sim=sim, which=which, related=related, released=released)


@pytest.fixture(scope="module")
def env():
    e = _integer_model()
    yield e
    e["model"].close()


def _bare(m, sel, pen=PEN):
    return dict(medium=m, users=[], penalties=pen, items=[dict(medium=a, matchedid=int(i)) for a, i in sel])


def _states(env, pen=PEN):
    w0 = env["which"][0]
    plus, minus = np.flatnonzero(w0 == 0), np.flatnonzero(w0 == 1)
    return [_bare(0, [(0, 17), (0, 4000)], pen), _bare(1, [(0, 23), (1, 99)], pen), _bare(0, [(0, 301), (0, 301), (1, 5)], pen),
            _bare(1, [], pen), _bare(0, [(0, plus[2]), (0, minus[2])], pen), _bare(0, [(1, 77)], pen)]


def test_pages_against_the_rerank_of_the_exact_window(env):
    from recommendersystem_amd import serve
    model = env["model"]
    states = _states(env)
    order = [ri.ordering_exact(st["medium"], env["sim"], st, BIG, env["released"][st["medium"]])[0] for st in states]
    assert order[0].size > 8400
    pags = [dict(offset=0, limit=10), dict(offset=1020, limit=7), dict(offset=8300, limit=10), dict(offset=10, limit=10),
            dict(offset=int(order[4].size), limit=10), dict(offset=8192, limit=1024)]
    got = serve.render_items(model, states, pags)
    for g, (st, pg) in enumerate(zip(states, pags)):
        m = st["medium"]
        page, total = got[g]
        assert total == order[g].size and page.dtype == np.int32
        win = ri.page_window(total, pg)
        if win is None:
            assert page.size == 0 and g == 4
            continue
        cand = order[g][win[0]:win[1]]
        pen = [[PEN[k] for k in ("decay", "mmr_penalty", "same_series_penalty", "related_penalty")]]
        ids, _ = model.rank_request(None, m, [cand], group=[0], partialk=[win[3]], penalties=pen, histories=[[]],
                                    scores=[np.zeros(cand.size, np.float32)])
        assert np.array_equal(page, ids[0][win[2] - 1:win[3]]), g
        assert page.size == min(win[3], cand.size) - (win[2] - 1)          # (1020, 7): the page is cut at the end of the ranked slice
    # one state alone gives its page of the mixed call; two identical calls return identical bytes
    alone = serve.render_items(model, [states[2]], pags[2])
    assert np.array_equal(alone[0][0], got[2][0]) and alone[0][1] == got[2][1]
    again = serve.render_items(model, states, pags)
    assert all(a[0].tobytes() == b[0].tobytes() and a[1] == b[1] for a, b in zip(got, again))


def test_default_penalties_give_the_orderings_slice(env):
    from recommendersystem_amd import serve
    pen = dict(decay=0.9, mmr_penalty=0.0, same_series_penalty=0.0, related_penalty=0.0)       # compute.jl `/add_item`
    states = _states(env, pen)
    # offsets that are multiples of their limits, as the site pages: such a page never straddles two ranked slices
    pags = [dict(offset=0, limit=25), dict(offset=1008, limit=24), dict(offset=9000, limit=50), dict(offset=1024, limit=1024),
            dict(offset=8200, limit=100), dict(offset=4096, limit=512)]
    got = serve.render_items(env["model"], states, pags)
    for st, pg, (page, total) in zip(states, pags, got):
        ids = ri.ordering_exact(st["medium"], env["sim"], st, BIG, env["released"][st["medium"]])[0]
        assert total == ids.size
        assert np.array_equal(page, ids[pg["offset"]:pg["offset"] + pg["limit"]])


def test_argument_errors_leave_outputs_untouched(env):
    import recommendersystem_amd as ra
    model = env["model"]
    L = ra.lib()

    def call(gm, off, lim, sel=None, cap=None, clear_related=False):
        ng = len(gm)
        gm, off, lim = np.asarray(gm, np.int32), np.asarray(off, np.int64), np.asarray(lim, np.int32)
        pen = np.tile(np.asarray([0.9, 0.25, 0.5, 0.5], np.float32), ng)
        cap = int(lim.clip(0).sum()) if cap is None else cap
        bufs = [np.full(max(cap, 1) + 8, 0x5A5A5A5A, np.int32), np.full(ng + 1, 0x5A5A5A5A5A5A5A5A, np.int64), np.full(ng, 0x5A5A5A5A, np.int32)]
        sp = (None, None, None)
        if sel is not None:
            o = np.asarray(sel[0], np.int64); a = np.asarray(sel[1], np.int32); b = np.asarray(sel[2], np.int32)
            keep = (o, a, b)
            sp = tuple(x.ctypes.data for x in keep)
        rc = L.rsys_render_items(model._h, ng, gm.ctypes.data, off.ctypes.data, lim.ctypes.data, pen.ctypes.data, *sp, bufs[0].ctypes.data, cap,
                                 bufs[1].ctypes.data, bufs[2].ctypes.data)
        return rc, all((x.view(np.int32) == 0x5A5A5A5A).all() for x in bufs)

    assert call([0, 1], [0, 0], [10, 10]) == (0, False)
    bad = [dict(gm=[0, 2], off=[0, 0], lim=[10, 10]),                                  # medium
           dict(gm=[0, 1], off=[0, 0], lim=[10, 0]),                                   # limit
           dict(gm=[0, 1], off=[0, 0], lim=[1025, 10]),
           dict(gm=[0, 1], off=[0, -1], lim=[10, 10]),                                 # offset
           dict(gm=[0, 1], off=[0, 0], lim=[10, 10], sel=([0, 2, 1], [0, 0], [5, 6])),  # malformed offsets
           dict(gm=[0, 1], off=[0, 0], lim=[10, 10], sel=([0, 1, 2], [0, 1], [BIG[0], 6])),   # id out of range
           dict(gm=[0, 1], off=[0, 0], lim=[10, 10], sel=([0, 1, 2], [0, 3], [5, 6])),  # medium of a selected item
           dict(gm=[0, 1], off=[0, 0], lim=[10, 10], cap=19)]                          # ids_cap below the sum of the limits
    for kw in bad:
        rc, clean = call(**kw)
        assert rc == -1 and clean, kw
    model.set_related(1, None)                                                         # a missing table
    rc, clean = call([0, 1], [0, 0], [10, 10])
    assert rc == -1 and clean
    model.set_related(1, env["related"]["1.related"])
    assert call([0, 1], [0, 0], [10, 10])[0] == 0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_render_items_between_training_steps_changes_nothing(dtype):
    """Deterministic mode: step -> load tables + render_items -> step gives the step -> step results bit for bit."""
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
    rng = np.random.default_rng(42)
    sim, _ = ri.integer_tables(rng, V)
    related = {f"{m}.related": rr.random_csc(rng, V[m], V[m], 0.05) for m in (0, 1)}
    states = [_bare(0, [(0, 3), (1, 4)]), _bare(1, [])]

    def run(with_request):
        model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
        model.load_state_dict(P)
        opt = ra.create_optimizer(model, dict(cfg, learning_rate=1e-2))
        model.set_loss_weights(TASK_W, 1)
        out = []
        for i, (d, mk) in enumerate(zip(batches, masks)):
            if i == 1 and with_request:
                serve.load_retrieval_tables(model, {}, sim, None)
                serve.load_ranking_tables(model, related)
                pages = serve.render_items(model, states, dict(offset=0, limit=10))
                assert all(p[0].size == 10 for p in pages)
            out.append(np.array(model(d, False, masks=mk), np.float32))
            out += [model.grad(n).copy() for n in names]
            opt.step(clip_max_norm=1.0)
        out += [model.get_parameter(n).copy() for n in names]
        model.close()
        return out

    a, b = run(False), run(True)
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _render_user(rng, V, n_events):
    items, ts = [], 1.2e9
    for _ in range(n_events):
        ts += float(rng.integers(10, 10 ** 6))
        y = int(rng.integers(0, 2))
        items.append({"medium": y, "matchedid": int(rng.integers(1, V[y])), "history_max_ts": ts, "status": int(rng.integers(0, 9)),
                      "rating": float(rng.integers(0, 11)), "progress": float(rng.random()), "history_status": -1, "history_rating": -1.0})
    return {"user": {"user": {"gender": [None, 0, 1][int(rng.integers(0, 3))], "source": int(rng.integers(0, 3))}, "items": items,
                     "timestamp": ts + 60.0}}


def test_render_exact_serves_every_state():
    """serve.render(..., exact=True) on states with and without users, V = (3000, 2000): where the default path is defined the pages are
    its pages and the totals the admissible counts; user-less states are serve.render_items's."""
    import recommendersystem_amd as ra
    from recommendersystem_amd import serve
    V = (3000, 2000)
    cfg = _cfg(V)
    cfg["forward"] = "inference"
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=4)
    model.init_weights(11)
    model.random_pretrained_embeddings(12)
    rng = np.random.default_rng(43)
    rel = rr.random_relations(rng, V, density=0.0005)
    sim = {f"embeddings.{m}": (0.3 * rng.standard_normal((64, V[m]))).astype(np.float32) for m in (0, 1)}
    sim.update({f"crossproject.{m}": (0.2 * rng.standard_normal((64, 64))).astype(np.float32) for m in (0, 1)})
    related = {f"{m}.related": rr.random_csc(rng, V[m], V[m], 0.005) for m in (0, 1)}
    released = {m: rng.random(V[m]) < 0.9 for m in (0, 1)}
    serve.load_retrieval_tables(model, rel, sim, released)
    serve.load_ranking_tables(model, related)

    def state(m, n_users, sel):
        users = [_render_user(rng, V, int(rng.integers(0, 12))) for _ in range(n_users)]
        return dict(medium=m, users=users, penalties=PEN, items=[dict(medium=a, matchedid=i) for a, i in sel])

    states = [state(0, 2, [(0, 5)]), state(1, 0, [(0, 7), (1, 9)]), state(1, 1, []), state(0, 0, []), state(0, 1, [(1, 3)])]
    pags = [dict(offset=0, limit=10), dict(offset=20, limit=10), dict(offset=1020, limit=7), dict(offset=1990, limit=50), dict(offset=10 ** 6, limit=5)]
    for st in states:
        m = st["medium"]
        for u in st["users"]:
            u["embeds"] = {f"{m}.retrieval": serve.predict(model, [u["user"]], "retrieval", m)[0][f"{m}.retrieval"]}
    with_users = [j for j, st in enumerate(states) if st["users"]]
    base = serve.render(model, [states[j] for j in with_users], [pags[j] for j in with_users])
    bare = [j for j, st in enumerate(states) if not st["users"]]
    items = serve.render_items(model, [states[j] for j in bare], [pags[j] for j in bare])
    exact = serve.render(model, states, pags, exact=True)
    for j, want in zip(with_users, base):
        st = states[j]
        adm = int((~rr.set_mask(st["medium"], rel, st, V, released=released[st["medium"]])).sum())
        assert exact[j][1] == adm == want[1]
        assert np.array_equal(exact[j][0], want[0]), j
    for j, want in zip(bare, items):
        assert np.array_equal(exact[j][0], want[0]) and exact[j][1] == want[1]
        assert want[0].size > 0
    with pytest.raises(ValueError):
        serve.render(model, states, pags)                                              # the default path still refuses user-less states
    with pytest.raises(ra.RsysError):
        model.retrieve_request(np.zeros((1, cfg["embed_dim"]), np.float32), 0, 5, group=[1])   # ... and so does the old entry point
    model.close()
