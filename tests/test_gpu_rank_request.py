"""GPU: ranking and diversity reranking of retrieved candidates on the device (rsys_rank_request: Inference/render.jl:335-435).  The greedy
loop alone bit for bit against the numpy restatement (tests/_render_rank_np.py) through rsys_op_rerank; the Gram matrix and ranking score
against fp64; the whole call's ids against the restatement fed the device's own Gram matrix and score; reproducibility, isolation from
training, `serve.render` end to end, and argument errors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_rank_np as rk  # noqa: E402
import _render_retrieval_np as rr  # noqa: E402

pytestmark = pytest.mark.gpu

DIM = 64
TASK_W = [0.05, 0.2, 0.3, 0.25]


def _bits(P):
    """bool [rows][n] -> int32 words [rows][ceil(n / 32)], bit i of row j = P[j, i]"""
    P = np.atleast_2d(P)
    rows, n = P.shape
    w = (n + 31) // 32
    out = np.zeros((rows, w), np.uint32)
    for i in range(n):
        out[:, i >> 5] |= P[:, i].astype(np.uint32) << np.uint32(i & 31)
    return out.view(np.int32)


def _op_rerank(r, G, pairs, flags, partialk, pen):
    from recommendersystem_amd._lib import check, lib
    L = lib()
    n = r.size
    k = min(partialk, n)
    host = [np.ascontiguousarray(r, np.float32), np.ascontiguousarray(G, np.float32), np.ascontiguousarray(_bits(pairs.T)),
            np.ascontiguousarray(_bits(flags[None, :])[0])]
    ptrs = []
    try:
        for a in host + [np.zeros(k, np.int32)]:
            p = C.c_void_p()
            check(L.rsys_dev_alloc(C.byref(p), max(a.nbytes, 4)))
            ptrs.append(p)
            check(L.rsys_dev_h2d(p, a.ctypes.data, a.nbytes))
        pv = np.ascontiguousarray(pen, np.float32)
        check(L.rsys_op_rerank(n, partialk, pv.ctypes.data, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4]))
        picks = np.empty(k, np.int32)
        check(L.rsys_dev_d2h(picks.ctypes.data, ptrs[4], picks.nbytes))
    finally:
        for p in ptrs:
            L.rsys_dev_free(p)
    return picks


def _case(rng, n, kind):
    r = rng.standard_normal(n).astype(np.float32)
    if kind == "ties":
        r = rng.integers(-3, 3, n).astype(np.float32)
    elif kind == "zeros":
        r = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        r[rng.random(n) < 0.2] = 1.0
    elif kind == "neginf":
        r[rng.random(n) < 0.7] = -np.inf
    elif kind == "nan":
        r[rng.random(n) < 0.05] = np.nan
        r[rng.random(n) < 0.05] = np.inf
    E = rng.standard_normal((n, 8)).astype(np.float32)
    G = E @ E.T
    G = np.triu(G) + np.triu(G, 1).T                      # symmetric, as the device's Gram matrix is
    if kind == "nan":
        j = rng.integers(0, n)
        G[j, :] = np.nan
        G[:, j] = np.nan
    pairs = rng.random((n, n)) < 4.0 / n
    np.fill_diagonal(pairs, rng.random(n) < 0.5)          # diagonal entries present and absent
    flags = rng.random(n) < 0.1
    return r, G.astype(np.float32), pairs, flags


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 1024])
def test_loop_alone_bit_for_bit(n):
    rng = np.random.default_rng(n)
    kinds = ["plain", "ties", "zeros", "neginf", "nan"]
    for kind in kinds:
        r, G, pairs, flags = _case(rng, n, kind)
        for partialk in sorted({1, max(1, n // 2), n, n + 7}):
            for decay in (0.0, 0.9, 1.0):
                pen = (decay, float(rng.choice([0.0, 0.3, -0.2])), float(rng.choice([0.0, 0.5, -1.0])), float(rng.choice([0.0, 0.25, -0.5])))
                if n >= 1000 and partialk not in (n // 2, n + 7) and kind != "neginf":
                    continue                              # (keep the largest sizes to a few long loops)
                got = _op_rerank(r, G, pairs, flags, partialk, pen)
                want = rk.reranking_given(r, G, pairs, flags, partialk, *pen)
                assert got.tolist() == want, (kind, partialk, pen)


def test_loop_repeats_picks_past_the_finite_scores():
    r = np.array([-np.inf, 2.0, -np.inf, 1.0], np.float32)
    G = np.zeros((4, 4), np.float32)
    no = np.zeros((4, 4), bool)
    got = _op_rerank(r, G, no, np.zeros(4, bool), 4, (1.0, 0.0, 0.0, 0.0)).tolist()
    assert got == rk.reranking_given(r, G, no, np.zeros(4, bool), 4, 1.0, 0.0, 0.0, 0.0) == [1, 3, 0, 0]


def _model(dtype, deterministic=False, name="hd64"):
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config(name, mask_rate=0.2, mask_topk=4)
    if deterministic:
        cfg["deterministic"] = True
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=4)
    model.load_state_dict(synth.make_params(cfg, 9, "test"))
    V = (cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"])
    return cfg, model, V


def _tables(model, rng, V, dim=DIM):
    from recommendersystem_amd import serve
    sim = {f"embeddings.{m}": (0.3 * rng.standard_normal((dim, V[m]))).astype(np.float32) for m in (0, 1)}
    related = {f"{m}.related": rr.random_csc(rng, V[m], V[m], 0.05) for m in (0, 1)}
    serve.load_retrieval_tables(model, {}, sim)
    serve.load_ranking_tables(model, related)
    return sim, related


def _bf16(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16
    return b.astype(np.uint32).view(np.float32)


def _states(rng, V, m, sizes):
    """one render state per candidate count: users with list items (duplicates, every status), penalties, candidates"""
    states, idxs = [], []
    for g, n in enumerate(sizes):
        st = rr.random_state(rng, V, m, n_users=int(rng.integers(1, 4)), n_items=40, n_selected=0)
        st["penalties"] = dict(decay=float(rng.choice([0.0, 0.9, 1.0])), mmr_penalty=float(rng.uniform(0, 0.5)),
                               same_series_penalty=float(rng.uniform(0, 2)), related_penalty=float(rng.uniform(-1, 1)))
        states.append(st)
        idxs.append(rng.choice(V[m], n, replace=False).astype(np.int32))
    return states, idxs


def _request(model, cfg, rng, m, states, idxs, partialk, registry=None):
    from recommendersystem_amd import serve
    D = cfg["embed_dim"]
    for st, c in zip(states, idxs):
        for u in st["users"]:
            u["embeds"] = {f"{m}.retrieval": rng.standard_normal(D).astype(np.float32),
                           f"{m}.ranking": rng.uniform(0, 10, c.size).astype(np.float32)}
    q, group, rm, hist, pen = serve.rank_arrays(states, idxs)
    rc, kc, mean = serve._registry_coefs(registry, m)
    return model.rank_request(q, m, idxs, group=group, r_masked=rm, partialk=partialk, penalties=pen, histories=hist, retrieval_coef=rc,
                              rating_coefs=kc, rating_mean=mean), (q, group, rm, hist, pen, rc, kc, mean)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_whole_call_against_the_restatement(dtype):
    cfg, model, V = _model(dtype)
    rng = np.random.default_rng(21)
    sim, related = _tables(model, rng, V)
    n0 = cfg["vocab_sizes"]["0_matchedid"]
    F = model.item_embeddings()
    registry = {"0.retrieval.coefs": np.array([0.7]), "0.rating.coefs": np.array([0.2, 0.9]), "0.rating_mean": 3.5,
                "1.rating.coefs": np.array([0.1, 1.1]), "1.rating_mean": 2.0}
    for m in (0, 1):
        Vm = V[m]
        sizes = [1, 7, min(64, Vm), min(65, Vm), Vm]
        states, idxs = _states(rng, V, m, sizes)
        partialk = [1, 3, 64, 100, Vm // 2]
        (ids, r), (q, group, rm, hist, pen, rc, kc, mean) = _request(model, cfg, rng, m, states, idxs, partialk, registry)
        Fm = F[:n0] if m == 0 else F[n0:]
        qq = q
        if dtype == "bf16":
            Fm, qq = _bf16(Fm), _bf16(q)
        G = model.rank_gram(m, idxs)
        for g, st in enumerate(states):
            members = np.flatnonzero(group == g)
            want = rk.ranking_fp64(Fm, qq[members], [rm[u] for u in members], idxs[g], rc, kc, mean)
            tol = (2e-2 if dtype == "bf16" else 1e-4) * np.maximum(1.0, np.abs(want)) * len(members)
            assert (np.abs(r[g] - want) <= tol).all(), (m, g, np.abs(r[g] - want).max())
            E = sim[f"embeddings.{m}"].T.astype(np.float64)[idxs[g]]
            G64 = E @ E.T
            assert np.array_equal(G[g], G[g].T)
            assert (np.abs(G[g] - G64) <= 1e-5 * (1.0 + np.abs(E) @ np.abs(E).T)).all()
            pairs = rk.pair_matrix(related[f"{m}.related"], idxs[g])
            flags = rk.related_flags(related[f"{m}.related"], idxs[g], st["users"], m)
            want_ids = idxs[g][rk.reranking_given(r[g], G[g], pairs, flags, partialk[g], *pen[g])]
            assert np.array_equal(ids[g], want_ids), (m, g)
    model.close()


def test_underflow_gives_minus_infinity():
    cfg, model, V = _model("fp32")
    rng = np.random.default_rng(22)
    _tables(model, rng, V)
    D = cfg["embed_dim"]
    n0 = cfg["vocab_sizes"]["0_matchedid"]
    F = model.item_embeddings()[:n0].astype(np.float64)
    q = np.zeros((1, D), np.float32)
    j = int(np.argmax(np.abs(F).sum(1)))
    q[0] = (np.sign(F[j]) * 400.0 / np.abs(F[j]).sum()).astype(np.float32)   # item j far above the others
    z = F @ q[0].astype(np.float64)
    lo = int(np.argmin(z))
    assert z[j] - z[lo] > 120                                                  # exp underflows in fp32 at the low item
    cand = np.array([j, lo], np.int32)
    _, r = model.rank_request(q, 0, [cand], r_masked=[np.zeros(2, np.float32)], rerank=False)
    assert np.isfinite(r[0][0]) and np.isneginf(r[0][1])
    _, r2 = model.rank_request(q, 0, [cand], r_masked=[np.zeros(2, np.float32)], retrieval_coef=1e-30, rerank=False)
    assert np.isneginf(r2[0][1])
    model.close()


def test_reproducible():
    cfg, model, V = _model("bf16")
    rng = np.random.default_rng(23)
    _tables(model, rng, V)
    states, idxs = _states(rng, V, 1, [50, 120, 200])
    a, args = _request(model, cfg, rng, 1, states, idxs, [10, 120, 300])
    q, group, rm, hist, pen = args[:5]
    b = model.rank_request(q, 1, idxs, group=group, r_masked=rm, partialk=[10, 120, 300], penalties=pen, histories=hist)
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert x.tobytes() == y.tobytes()
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_request_between_training_steps_changes_nothing(dtype):
    """Deterministic mode: step -> load tables + rank_request -> step gives the step -> step results bit for bit."""
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config("hd64", mask_rate=0.2, deterministic=True)
    V = (cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"])
    P = synth.make_params(cfg, 3, "test")
    rows = 4
    batches = [synth.make_batch(cfg, rows, 40 + i) for i in range(2)]
    masks = [synth.make_masks(cfg, rows, 50 + i) for i in range(2)]
    names = synth.trainable_names(cfg)

    def run(rank):
        model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
        model.load_state_dict(P)
        opt = ra.create_optimizer(model, dict(cfg, learning_rate=1e-2))
        model.set_loss_weights(TASK_W, 1)
        out = []
        for i, (d, mk) in enumerate(zip(batches, masks)):
            if i == 1 and rank:
                rng = np.random.default_rng(24)
                _tables(model, rng, V)
                states, idxs = _states(rng, V, 0, [30, 100])
                _request(model, cfg, rng, 0, states, idxs, [5, 100])
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
    return {"user": {"user": {"gender": None, "source": 2}, "items": items, "timestamp": ts + 60.0}}


def test_render_end_to_end_and_chunking():
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import serve
    cfg = synth.make_config("hd64", mask_rate=0.2, mask_topk=4)
    cfg["forward"] = "inference"
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=4)
    model.load_state_dict(synth.make_params(cfg, 31, "test"))
    V = (cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"])
    rng = np.random.default_rng(25)
    rel = rr.random_relations(rng, V, density=0.01)
    sim = {f"embeddings.{m}": (0.3 * rng.standard_normal((DIM, V[m]))).astype(np.float32) for m in (0, 1)}
    related = {f"{m}.related": rr.random_csc(rng, V[m], V[m], 0.05) for m in (0, 1)}
    serve.load_retrieval_tables(model, rel, sim)
    serve.load_ranking_tables(model, related)
    registry = {"1.rating.coefs": np.array([0.3, 0.8]), "1.rating_mean": 4.0, "1.retrieval.coefs": np.array([0.5])}
    m = 1
    D = cfg["embed_dim"]
    for pag in ({"offset": 0, "limit": 10}, {"offset": 25, "limit": 10}, {"offset": 5, "limit": 7}, {"offset": 10 ** 6, "limit": 10}):
        users = [_render_user(rng, V, int(rng.integers(3, 12))) for _ in range(2)]
        for u in users:
            u["embeds"] = {f"{m}.retrieval": serve.predict(model, [u["user"]], "retrieval", m)[0][f"{m}.retrieval"]}
        st = dict(medium=m, items=[], users=users, penalties=dict(decay=0.9, mmr_penalty=0.2, same_series_penalty=0.5, related_penalty=0.3))
        (ids, total), = serve.render(model, [st], pag, registry)
        # the same steps on the host: retrieval, the page's slice, the forward's values, the restatement on the device's score
        ret = serve.retrieval(model, [st], k=8192)[0][0]
        assert total == ret.size
        win = serve.page_window(ret.size, pag)
        if win is None:
            assert ids.size == 0
            continue
        cand = ret[win[0]:win[1]]
        ranked = {u: np.asarray(users[u]["embeds"][f"{m}.ranking"]).copy() for u in range(2)}
        half = cfg["max_sequence_length"] - cfg["max_sequence_length"] // 2       # candidates one ranking forward holds
        for u in users:
            want = []
            for c0 in range(0, cand.size, half):
                want += serve.predict(model, [dict(u["user"], ranking_items=[int(x) for x in cand[c0:c0 + half]])], "ranking", m)[0][f"{m}.ranking"]
            np.testing.assert_allclose(np.asarray(u["embeds"][f"{m}.ranking"], np.float32), np.asarray(want, np.float32), rtol=1e-5, atol=1e-5)
        r = serve.ranking(model, [st], [cand], registry)[0]
        G = model.rank_gram(m, [cand])[0]
        p = st["penalties"]
        picks = rk.reranking_given(r, G, rk.pair_matrix(related[f"{m}.related"], cand),
                                   rk.related_flags(related[f"{m}.related"], cand, users, m), win[3], p["decay"], p["mmr_penalty"],
                                   p["same_series_penalty"], p["related_penalty"])
        assert np.array_equal(ids, cand[picks][win[2] - 1:win[3]])
        assert np.array_equal(serve.reranking(model, [st], [cand], [r], win[3])[0], cand[picks])
        # chunked ranking forward: the same values
        (ids2, total2), = serve.render(model, [st], pag, registry, max_ranking_items=3)
        for u in range(2):
            np.testing.assert_allclose(np.asarray(users[u]["embeds"][f"{m}.ranking"]), ranked[u], rtol=1e-5, atol=1e-5)
        assert total2 == total
    model.close()


def test_argument_errors():
    import recommendersystem_amd as ra
    from recommendersystem_amd import _lib
    cfg, model, V = _model("fp32")
    rng = np.random.default_rng(26)
    D = cfg["embed_dim"]
    q = rng.standard_normal((2, D)).astype(np.float32)
    cand = [np.arange(1, 11, dtype=np.int32), np.arange(20, 25, dtype=np.int32)]
    rm = [np.zeros(10, np.float32), np.zeros(5, np.float32)]
    pen = np.zeros((2, 4), np.float32)
    call = lambda **kw: model.rank_request(**{**dict(queries=q, medium=0, candidates=cand, group=[0, 1], r_masked=rm, partialk=[3, 3],
                                                     penalties=pen), **kw})
    with pytest.raises(ra.RsysError):                                      # no similarity / related table yet
        call()
    model.rank_request(q, 0, cand, group=[0, 1], r_masked=rm, rerank=False)  # ranking alone needs neither
    sim = {f"embeddings.{m}": rng.standard_normal((DIM, V[m])).astype(np.float32) for m in (0, 1)}
    from recommendersystem_amd import serve
    serve.load_retrieval_tables(model, {}, sim)
    with pytest.raises(ra.RsysError):                                      # related still missing
        call()
    serve.load_ranking_tables(model, {"0.related": rr.random_csc(rng, V[0], V[0], 0.05)})
    call()
    bad = [
        dict(candidates=[np.arange(V[0] + 1, dtype=np.int32) % V[0], cand[1]]),   # duplicate ids (and n > V_m)
        dict(candidates=[np.array([1, 2, 1], np.int32), cand[1]], r_masked=[np.zeros(3, np.float32), rm[1]]),
        dict(candidates=[np.array([1, V[0]], np.int32), cand[1]], r_masked=[np.zeros(2, np.float32), rm[1]]),
        dict(candidates=[np.array([-1, 2], np.int32), cand[1]], r_masked=[np.zeros(2, np.float32), rm[1]]),
        dict(partialk=[0, 3]),
        dict(r_masked=[np.zeros(9, np.float32), rm[1]]),                     # ragged r_masked of the wrong length
        dict(group=[0, 0], r_masked=[rm[0], rm[0]]),                         # group 1 has no user
        dict(histories=[[(0, V[0], 7)], []]),                                # list id out of range
        dict(medium=2),
    ]
    for kw in bad:
        with pytest.raises((ra.RsysError, ValueError)):
            call(**kw)
    big = [np.arange(1025, dtype=np.int32) % V[0]]
    with pytest.raises(ra.RsysError):                                      # n_g > 1024
        model.rank_request(q[:1], 0, big, r_masked=[np.zeros(1025, np.float32)], partialk=[3], penalties=pen[:1])
    L = ra.lib()
    ip, ix, d, (nr, nc) = rr.random_csc(rng, V[0], V[0], 0.05)
    bad_d = d.copy(); bad_d[0] = -1.0
    for args in ((0, nr + 1, ip, ix, d), (0, nr, ip, ix, bad_d), (2, nr, ip, ix, d)):
        with pytest.raises(ra.RsysError):
            _lib.check(L.rsys_rank_related_set(model._h, args[0], args[1], np.ascontiguousarray(args[2], np.int64).ctypes.data,
                                               np.ascontiguousarray(args[3], np.int32).ctypes.data,
                                               np.ascontiguousarray(args[4], np.float32).ctypes.data))
    call()                                                                 # still usable
    model.set_item_similarity(0, None)
    with pytest.raises(ra.RsysError):                                      # similarity table cleared
        call()
    model.close()
