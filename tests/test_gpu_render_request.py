"""GPU: rsys_render_request / serve.render_users -- a page from raw histories in one device pipeline.  The device's own
intermediates (query buffer, retrieved ids, assembled ranking rows, r_masked, ranking scores, pick order) are read through the debug
channel and checked stage by stage: assembly bit for bit against serve.build_batch, the two forwards against the staged path
(serve.predict) run on the same model, every downstream stage bit for bit given the device's own inputs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _adapter_bank_util as ab  # noqa: E402
import _render_rank_np as rk  # noqa: E402
import _render_retrieval_np as rr  # noqa: E402

pytestmark = pytest.mark.gpu

DIM = 64
TASK_W = [0.05, 0.2, 0.3, 0.25]
COLS = ("userid", "rope_input_pos", "token_mask_ids", "gender", "source", "matchedid", "status", "time", "rating", "progress")
# Stage comparisons against the staged path (serve.predict).  fp32: rtol = atol = 1e-5, the bound of the existing chunking test for the
# same forward.  bf16: the issue's bound is twice the largest |difference| of serve.predict between a user run alone and the same user
# at each position of a four-row batch.  That figure was measured on the commit before this change, with this file's users, on the bank
# model and on the plain model: 0.0 for the retrieval embedding and 0.0 for the ranking values.  Twice zero is zero, so
# bf16 asserts equality.  `test_staged_forward_is_row_count_independent` repeats the measurement on the staged path and asserts the zero.


def _row_count_diff(model, cfg, V, states):
    """serve.predict on one row vs the same user inside a four-row batch (every position), per task"""
    from recommendersystem_amd import serve
    S = cfg["max_sequence_length"]
    rng = np.random.default_rng(77)
    worst = {"retrieval": 0.0, "ranking": 0.0}
    everyone = [u["user"] for st in states for u in st["users"]]
    for st in states:
        m = int(st["medium"])
        cands = [int(x) for x in rng.choice(np.arange(1, V[m]), S - S // 2, replace=False)]
        others = [dict(everyone[i % len(everyone)], ranking_items=cands) for i in range(3)]           # (three more rows: a four-row batch)
        for u in st["users"]:
            req = dict(u["user"], ranking_items=cands)
            for task in ("retrieval", "ranking"):
                key = f"{m}.{task}"
                one = np.asarray(serve.predict(model, [req], task, m)[0][key], np.float32)
                for pos in range(4):
                    four = serve.predict(model, others[:pos] + [req] + others[pos:], task, m)[pos][key]
                    worst[task] = max(worst[task], float(np.abs(one - np.asarray(four, np.float32)).max()))
    print(f"one row vs four rows (staged path): max |diff| retrieval {worst['retrieval']:.3e} ranking {worst['ranking']:.3e}")
    return worst


def _tol(dtype, task):
    if dtype == "fp32":
        return dict(rtol=1e-5, atol=1e-5)
    return dict(rtol=0.0, atol=0.0)


def _close(got, want, dtype, task, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    diff = float(np.abs(got - want).max()) if got.size else 0.0
    print(f"{what} [{dtype}] max |diff| {diff:.3e}")
    tol = _tol(dtype, task)
    if tol["atol"] == 0.0 and tol["rtol"] == 0.0:
        assert np.array_equal(got, want), (what, diff)
    else:
        np.testing.assert_allclose(got, want, **tol)


def _cfg():
    from oracle import synth
    cfg = synth.make_config("hd64", mask_rate=0.2, mask_topk=4)
    cfg["forward"] = "inference"
    return cfg


def _model(kind, dtype, max_rows=4, seed=31):
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import serve
    cfg = _cfg()
    P = synth.make_params(cfg, seed, "test")
    if kind == "bank":
        blobs = ab.finetune_blobs(cfg, P, ab.make_adapters(cfg, 4, 70))
        model = serve.get_models(blobs[0], blobs, cfg, dtype=dtype, max_rows=max_rows)
    else:
        model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=max_rows)
        model.load_state_dict(P)
    V = (cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"])
    return cfg, model, V


def _tables(model, V, seed=25, released=None):
    from recommendersystem_amd import serve
    rng = np.random.default_rng(seed)
    rel = rr.random_relations(rng, V, density=0.01)
    sim = {f"embeddings.{m}": (0.3 * rng.standard_normal((DIM, V[m]))).astype(np.float32) for m in (0, 1)}
    sim.update({f"crossproject.{m}": (0.2 * rng.standard_normal((DIM, DIM))).astype(np.float32) for m in (0, 1)})
    related = {f"{m}.related": rr.random_csc(rng, V[m], V[m], 0.05) for m in (0, 1)}
    serve.load_retrieval_tables(model, rel, sim, released)
    serve.load_ranking_tables(model, related)
    return related


def _render_user(rng, V, n_events):
    items, ts = [], 1.2e9
    for _ in range(n_events):
        ts += float(rng.integers(10, 10 ** 6))
        y = int(rng.integers(0, 2))
        items.append({"medium": y, "matchedid": int(rng.integers(1, V[y])), "history_max_ts": ts, "status": int(rng.integers(0, 9)),
                      "rating": float(rng.integers(0, 11)), "progress": float(rng.random()), "history_status": -1, "history_rating": -1.0})
    return {"user": {"user": {"gender": [None, 0, 1][int(rng.integers(0, 3))], "source": int(rng.integers(0, 3))}, "items": items,
                     "timestamp": ts + 60.0}}


def _state(rng, V, m, n_users, n_selected, long_history=False):
    users = [_render_user(rng, V, int(rng.integers(40, 80)) if long_history and u == 0 else int(rng.integers(0, 12))) for u in range(n_users)]
    items = [dict(medium=int(rng.integers(0, 2)), matchedid=0) for _ in range(n_selected)]
    for a in items:
        a["matchedid"] = int(rng.integers(1, V[a["medium"]]))
    return dict(medium=m, items=items, users=users,
                penalties=dict(decay=float(rng.choice([0.0, 0.9, 1.0])), mmr_penalty=float(rng.uniform(0, 0.5)),
                               same_series_penalty=float(rng.uniform(0, 2)), related_penalty=float(rng.uniform(-1, 1))))


def _request(seed=40):
    """states of both media with 1-3 users, with and without selected items, one user with a history longer than a ranking row keeps;
    paginations: a first page, a second page, a limit that does not divide 1024, an offset past the end"""
    cfg = _cfg()
    V = (cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"])
    rng = np.random.default_rng(seed)
    states = [_state(rng, V, 1, 2, 0), _state(rng, V, 0, 1, 2), _state(rng, V, 1, 3, 1, long_history=True), _state(rng, V, 0, 2, 0),
              _state(rng, V, 1, 1, 3)]
    pags = [{"offset": 0, "limit": 10}, {"offset": 10, "limit": 10}, {"offset": 5, "limit": 7}, {"offset": 10 ** 6, "limit": 10},
            {"offset": 21, "limit": 7}]
    registry = {"1.rating.coefs": np.array([0.3, 0.8]), "1.rating_mean": 4.0, "1.retrieval.coefs": np.array([0.5]),
                "0.rating.coefs": np.array([0.2, 0.9]), "0.rating_mean": 3.5}
    return states, pags, registry


def _kept(model, cfg, states):
    """the last request's intermediates, shaped"""
    S, D = cfg["max_sequence_length"], cfg["embed_dim"]
    k = {"forwards": model.render_kept("forwards"), "queries": model.render_kept("queries").reshape(-1, D),
         "counts": model.render_kept("ret.counts"), "rows": model.render_kept("rows").reshape(-1, 6),
         "groups": model.render_kept("groups").reshape(-1, 6), "rm_users": model.render_kept("rm_users").reshape(-1, 3),
         "r_masked": model.render_kept("r_masked"), "r": model.render_kept("r"), "picks": model.render_kept("picks"),
         "token_index": model.render_kept("token_index")}
    ids = model.render_kept("ret.ids")
    k["ids"] = np.split(ids, np.cumsum(k["counts"])[:-1])
    k["batch"] = {c: model.render_kept(f"batch.{c}").reshape(-1, S) for c in COLS}
    k["users"] = [(g, u) for g, st in enumerate(states) for u in st["users"]]
    return k


def _check_request(model, cfg, V, related, states, pags, registry, dtype, out):
    """tests 1-3 of the issue on the intermediates of the request that returned `out`"""
    from recommendersystem_amd import serve
    S = cfg["max_sequence_length"]
    n0 = V[0]
    chunk, mul = S - S // 2, S // 2
    k = _kept(model, cfg, states)
    users = k["users"]
    group = np.array([g for g, _ in users], np.int32)
    medium = [int(st["medium"]) for st in states]
    # ---- retrieval forward against the staged path (2)
    want_q = [serve.predict(model, [u["user"]], "retrieval", medium[g])[0][f"{medium[g]}.retrieval"] for g, u in users]
    _close(k["queries"], want_q, dtype, "retrieval", "query buffer vs serve.predict")
    # ---- retrieval given the device's own queries, bit for bit (3)
    for m in (0, 1):
        gs = [g for g in range(len(states)) if medium[g] == m]
        us = [i for i, (g, _) in enumerate(users) if medium[g] == m]
        if not gs:
            continue
        hist = [[(int(x["medium"]), int(x["matchedid"]), int(x["status"])) for x in users[i][1]["user"]["items"]] for i in us]
        sel = [[(int(a["medium"]), int(a["matchedid"])) for a in states[g]["items"]] for g in gs]
        kk = min(V[m], 8192)
        ids, _, counts = model.retrieve_request(k["queries"][us], m, kk, group=[gs.index(group[i]) for i in us], histories=hist, selected=sel)
        for j, g in enumerate(gs):
            assert counts[j] == k["counts"][g] == out[g][1], (g, counts[j], k["counts"][g], out[g][1])
            assert np.array_equal(ids[j, :counts[j]], k["ids"][g]), g
    # ---- the page windows and the ranking rows (1)
    active = {int(r[0]): r for r in k["groups"]}
    rows_seen = 0
    cand_of = {}
    for g, st in enumerate(states):
        win = serve.page_window(int(k["counts"][g]), pags[g])
        if win is None:
            assert g not in active and out[g][0].size == 0
            continue
        rec = active[g]
        cand_of[g] = k["ids"][g][win[0]:win[1]]
        assert (rec[1], rec[3], rec[4], rec[5]) == (medium[g], win[1] - win[0], win[2], win[3])
    rm_first = {int(u): (int(o), int(n)) for u, o, n in k["rm_users"]}
    tok_at = 0
    waves = {}
    for row in k["rows"]:
        waves.setdefault(int(row[5]), []).append(row)
    assert all(len(w) <= model.max_rows for w in waves.values())
    assert k["forwards"][1] == len(waves)
    for wave in sorted(waves):
        for row in waves[wave]:
            ui, g, c0_slot, ncand, wrow = (int(x) for x in row[:5])
            assert g == group[ui] and g in cand_of
            m = medium[g]
            first = c0_slot - int(active[g][2])                        # first candidate of the chunk within the group's window
            cand = cand_of[g][first:first + ncand]
            assert first % chunk == 0 and ncand == min(chunk, cand_of[g].size - first)
            req = dict(users[ui][1]["user"], ranking_items=[int(x) for x in cand])
            d = serve.build_batch([req], "ranking", m, n0, mul, S - mul)
            for c in COLS:
                assert k["batch"][c][rows_seen].tobytes() == d[c][0].tobytes(), (c, ui, first)
            index, _ = serve._selected_tokens([req], "ranking", S, mul)
            got = k["token_index"][tok_at:tok_at + ncand] - wrow * 2 * S
            assert got.tolist() == index, (ui, first)
            # ---- ranking forward against the staged path on the device's candidates (2)
            want = serve.predict(model, [req], "ranking", m, mul, S - mul)[0][f"{m}.ranking"]
            o = rm_first[ui][0] + first
            _close(k["r_masked"][o:o + ncand], want, dtype, "ranking", f"r_masked vs serve.predict (user {ui}, chunk {first})")
            tok_at += ncand
            rows_seen += 1
    n_rows = sum(len(st["users"]) * len(serve.render_row_plan(cand_of[g].size, 0, S)) for g, st in enumerate(states) if g in cand_of)
    assert rows_seen == n_rows == k["rows"].shape[0] and tok_at == k["token_index"].size
    # ---- ranking, reranking and the page given their inputs, bit for bit (3)
    for m in (0, 1):
        gs = [g for g in sorted(cand_of) if medium[g] == m]
        if not gs:
            continue
        us = [i for i, (g, _) in enumerate(users) if g in gs]
        rc, kc, mean = serve._registry_coefs(registry, m)
        rm = [k["r_masked"][rm_first[i][0]:rm_first[i][0] + rm_first[i][1]] for i in us]
        _, r = model.rank_request(k["queries"][us], m, [cand_of[g] for g in gs], group=[gs.index(group[i]) for i in us], r_masked=rm,
                                  retrieval_coef=rc, rating_coefs=kc, rating_mean=mean, rerank=False)
        G = model.rank_gram(m, [cand_of[g] for g in gs])
        for j, g in enumerate(gs):
            _, _, c0, n, sidx, eidx = (int(x) for x in active[g])
            dev_r = k["r"][c0:c0 + n]
            assert dev_r.tobytes() == r[j].tobytes(), g
            p = states[g]["penalties"]
            picks = rk.reranking_given(dev_r, G[j], rk.pair_matrix(related[f"{m}.related"], cand_of[g]),
                                       rk.related_flags(related[f"{m}.related"], cand_of[g], states[g]["users"], m), eidx, p["decay"],
                                       p["mmr_penalty"], p["same_series_penalty"], p["related_penalty"])
            assert k["picks"][c0:c0 + eidx].tolist() == list(picks), g
            assert np.array_equal(out[g][0], cand_of[g][picks][sidx - 1:eidx]), g
    return k


@pytest.mark.parametrize("kind", ["bank", "plain"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stages_against_the_staged_path(kind, dtype):
    from recommendersystem_amd import serve
    cfg, model, V = _model(kind, dtype)
    related = _tables(model, V)
    states, pags, registry = _request()
    model.render_keep(True)
    out = serve.render_users(model, states, pags, registry)
    assert [o[0].dtype for o in out] == [np.int32] * len(states)
    k = _check_request(model, cfg, V, related, states, pags, registry, dtype, out)
    n_users = sum(len(st["users"]) for st in states)
    assert k["forwards"][0] == -(-n_users // model.max_rows)
    assert out[3][0].size == 0 and out[3][1] == k["counts"][3]            # the offset past the end: (empty, total), no ranking row
    assert not (k["rows"][:, 1] == 3).any()
    assert all(o[0].size for g, o in enumerate(out) if g != 3)
    # the staged sequence on the same model returns the same pages (a row's result does not depend on the rows beside it)
    for g, st in enumerate(states):
        m = int(st["medium"])
        for u in st["users"]:
            u["embeds"] = {f"{m}.retrieval": serve.predict(model, [u["user"]], "retrieval", m)[0][f"{m}.retrieval"]}
    staged = serve.render(model, states, pags, registry)
    for a, b in zip(out, staged):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_chunk_rows_share_one_forward(dtype):
    """a window of more than S - S // 2 candidates, 2 users, max_rows = 4: 2 x 2 chunk rows in ONE ranking forward"""
    from recommendersystem_amd import serve
    cfg, model, V = _model("bank", dtype, max_rows=4)
    S = cfg["max_sequence_length"]
    rng = np.random.default_rng(41)
    states = [_state(rng, V, 1, 2, 1)]
    # 48 admissible items: the released set is 48 of the items no other rule masks (the rules restated on the host; the relations are
    # the ones `_tables` draws first from its seed)
    rel = rr.random_relations(np.random.default_rng(25), V, density=0.01)
    free = np.flatnonzero(~rr.set_mask(1, rel, states[0], V))
    assert free.size >= 48, free.size
    released = {1: rng.choice(free, 48, replace=False)}
    related = _tables(model, V, seed=25, released=released)
    pags = [{"offset": 35, "limit": 10}]
    registry = {"1.rating.coefs": np.array([0.3, 0.8]), "1.rating_mean": 4.0}
    model.render_keep(True)
    out = serve.render_users(model, states, pags, registry)
    k = _check_request(model, cfg, V, related, states, pags, registry, dtype, out)
    n = int(k["groups"][0][3])
    assert S - S // 2 < n <= 2 * (S - S // 2), n                              # (the setup: two chunks per user)
    assert k["rows"].shape[0] == 4 and k["forwards"].tolist() == [1, 1]
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_waves_give_the_results_of_one_large_batch(dtype):
    from recommendersystem_amd import serve
    states, pags, registry = _request(seed=42)
    res = {}
    for max_rows in (32, 2):
        cfg, model, V = _model("bank", dtype, max_rows=max_rows)
        related = _tables(model, V)
        model.render_keep(True)
        out = serve.render_users(model, states, pags, registry)
        k = _check_request(model, cfg, V, related, states, pags, registry, dtype, out)
        res[max_rows] = (out, k)
        model.close()
    (o2, k2), (o32, k32) = res[2], res[32]
    assert k2["forwards"][0] > 1 and k2["forwards"][1] > 1 and k32["forwards"].tolist() == [1, 1]
    # a row's result does not depend on the rows beside it: everything is equal, in both dtypes
    for key in ("queries", "counts", "r_masked", "r", "picks"):
        assert k2[key].tobytes() == k32[key].tobytes(), key
    assert all(np.array_equal(a, b) for a, b in zip(k2["ids"], k32["ids"]))
    for a, b in zip(o2, o32):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]


@pytest.mark.parametrize("kind", ["bank", "plain"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_staged_forward_is_row_count_independent(kind, dtype):
    """the measurement behind the bf16 bound, on the staged path alone: one row against the same user in a four-row batch"""
    cfg, model, V = _model(kind, dtype)
    states, _, _ = _request()
    assert _row_count_diff(model, cfg, V, states) == {"retrieval": 0.0, "ranking": 0.0}
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_a_full_slice_of_1024_candidates(dtype):
    """the chunker at max_items_to_rank: a catalogue large enough for a 1024-candidate window, S - S // 2 = 32 candidates per row, so
    32 rows per user in 16 waves of 4 rows"""
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import serve
    cfg = _cfg()
    cfg["vocab_sizes"] = dict(cfg["vocab_sizes"], **{"1_matchedid": 1500})
    V = (cfg["vocab_sizes"]["0_matchedid"], 1500)
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=4)
    model.load_state_dict(synth.make_params(cfg, 33, "test"))
    rng = np.random.default_rng(46)
    empty = lambda r, c: (np.zeros(c + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), (r, c))
    rel = {f"{m}.{k}": empty(V[m], V[1 - m] if k == "adaptations" else V[m]) for m in (0, 1) for k in serve.RELATION_KINDS}
    sim = {f"embeddings.{m}": (0.3 * rng.standard_normal((DIM, V[m]))).astype(np.float32) for m in (0, 1)}
    related = {f"{m}.related": rr.random_csc(rng, V[m], V[m], 0.005) for m in (0, 1)}
    serve.load_retrieval_tables(model, rel, sim)
    serve.load_ranking_tables(model, related)
    states = [_state(rng, V, 1, 2, 0)]
    pags = [{"offset": 8, "limit": 8}]                                        # max_items_to_rank = 1024 - 1024 % 8 = 1024
    model.render_keep(True)
    out = serve.render_users(model, states, pags, None)
    k = _check_request(model, cfg, V, related, states, pags, None, dtype, out)
    S = cfg["max_sequence_length"]
    assert int(k["groups"][0][3]) == 1024 and out[0][0].size == 8
    assert k["rows"].shape[0] == 2 * len(serve.render_row_plan(1024, 0, S)) == 64 and k["forwards"].tolist() == [1, 16]
    model.close()


def test_reproducible():
    from recommendersystem_amd import serve
    cfg, model, V = _model("bank", "bf16")
    _tables(model, V)
    states, pags, registry = _request(seed=43)
    model.render_keep(True)
    keys = ["queries", "ret.ids", "ret.counts", "r_masked", "r", "picks", "token_index", "batch.matchedid", "batch.time", "rows", "groups"]
    a = serve.render_users(model, states, pags, registry)
    ka = [model.render_kept(x).tobytes() for x in keys]
    b = serve.render_users(model, states, pags, registry)
    kb = [model.render_kept(x).tobytes() for x in keys]
    assert ka == kb
    for x, y in zip(a, b):
        assert x[0].tobytes() == y[0].tobytes() and x[1] == y[1]
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_request_between_training_steps_changes_nothing(dtype):
    """Deterministic mode: step -> load tables + render_users -> step gives the step -> step results bit for bit."""
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

    def run(with_request):
        model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
        model.load_state_dict(P)
        opt = ra.create_optimizer(model, dict(cfg, learning_rate=1e-2))
        model.set_loss_weights(TASK_W, 1)
        out = []
        for i, (d, mk) in enumerate(zip(batches, masks)):
            if i == 1 and with_request:
                _tables(model, V)
                states, pags, registry = _request(seed=44)
                pages = serve.render_users(model, states, pags, registry)
                assert any(p[0].size for p in pages)
            out.append(np.array(model(d, False, masks=mk), np.float32))
            out += [model.grad(n).copy() for n in names]
            opt.step(clip_max_norm=1.0)
        out += [model.get_parameter(n).copy() for n in names]
        model.close()
        return out

    a, b = run(False), run(True)
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_argument_errors():
    import recommendersystem_amd as ra
    from recommendersystem_amd import serve
    cfg, model, V = _model("bank", "fp32")
    _tables(model, V)
    states, pags, registry = _request(seed=45)
    S, n0 = cfg["max_sequence_length"], V[0]
    args = serve.render_pack(states, pags, S, n0, registry, model.adapter_slots)
    good_pages, good_totals = model.render_request(**args)
    ng, nu = len(states), len(args["group"])

    def untouched(mdl=None, base=None, **kw):
        """the call fails with RSYS_ERR_ARG and writes nothing: the wrapper's output buffers are filled with a sentinel first"""
        import ctypes as C
        from recommendersystem_amd import _lib
        mdl = model if mdl is None else mdl
        a = {**(args if base is None else base), **kw}
        seen = {}
        real = _lib.lib().rsys_render_request

        class Spy:
            def __getattr__(self, name):
                return getattr(_lib.lib(), name) if name != "rsys_render_request" else call

        def call(*p):
            ids, cap, ioff, total = p[-4:]
            n_g = p[1]
            bufs = [(ids, max(cap, 1) * 4), (ioff, (n_g + 1) * 8), (total, max(n_g, 1) * 4)]
            for ptr, nbytes in bufs:
                C.memset(ptr, 0x5A, nbytes)
            rc = real(*p)
            seen["rc"] = rc
            seen["clean"] = all(C.string_at(ptr, nbytes) == b"\x5a" * nbytes for ptr, nbytes in bufs)
            return rc

        from recommendersystem_amd import model as model_mod
        old = model_mod.lib
        model_mod.lib = lambda: Spy()
        try:
            with pytest.raises(ra.RsysError):
                mdl.render_request(**a)
        finally:
            model_mod.lib = old
        assert seen["rc"] == -1 and seen["clean"], (kw.keys(), seen)

    untouched(group_medium=[2] + list(args["group_medium"][1:]))                     # bad medium
    untouched(group=[0] * nu)                                                        # groups without users
    untouched(adapter_slots=[0, 1, 2, 6])                                            # a slot that was never loaded
    untouched(limits=[0] + list(args["limits"][1:]))                                 # limit < 1
    untouched(limits=[1025] + list(args["limits"][1:]))
    untouched(offsets=[-1] + list(args["offsets"][1:]))
    untouched(histories=[[(0, V[0], 7)]] + args["histories"][1:])                    # list id out of range
    untouched(selected=[[(1, V[1])]] + args["selected"][1:])                         # selected id out of range
    untouched(retrieval_token=np.full(nu, 2 * S, np.int32))
    desc = args["user_desc"].copy(); desc[0, 0] = S // 2 + 1
    untouched(user_desc=desc)                                                        # a prefix longer than a ranking row keeps
    bad = {c: v.copy() for c, v in args["ranking_prefix"].items()}
    i = int(np.argmax(args["user_desc"][:, 0]))
    bad["matchedid"][i, 0] = V[0] + V[1]
    untouched(ranking_prefix=bad)                                                    # an index path of the prefix out of range
    model.clear_adapter(3)
    untouched()                                                                      # an incomplete adapter slot ("1.ranking")
    # malformed offsets reach the library only through the raw call: the wrapper builds them itself
    import ctypes as C
    from recommendersystem_amd import _lib
    from recommendersystem_amd.model import triples_csr
    model.load_adapter(3, ab.make_adapters(cfg, 1, 90)[0])
    pages, totals = model.render_request(**args)
    assert len(pages) == len(good_pages) and totals.shape == good_totals.shape          # (works again: slot 3 holds an adapter)
    gm = np.asarray(args["group_medium"], np.int32); off = np.asarray(args["offsets"], np.int64); lim = np.asarray(args["limits"], np.int32)
    pen = np.ascontiguousarray(args["penalties"], np.float32); gp = np.asarray(args["group"], np.int32)
    rb, keep_r = model._c_rows(args["retrieval_rows"], nu, S)
    pb, keep_p = model._c_rows(args["ranking_prefix"], nu, args["prefix_stride"])
    tok = np.asarray(args["retrieval_token"], np.int32); desc = np.ascontiguousarray(args["user_desc"], np.int32)
    ts = np.asarray(args["user_ts"], np.float64)

    def raw(h, sl, word):
        ids = np.full(int(lim.sum()), 0x5A5A5A5A, np.int32); ioff = np.full(ng + 1, 0x5A5A5A5A, np.int64); total = np.full(ng, 0x5A5A5A5A, np.int32)
        rc = _lib.lib().rsys_render_request(model._h, ng, gm.ctypes.data, off.ctypes.data, lim.ctypes.data, pen.ctypes.data, nu, gp.ctypes.data,
                                            C.byref(rb), tok.ctypes.data, C.byref(pb), args["prefix_stride"], desc.ctypes.data, ts.ctypes.data,
                                            None, *(a.ctypes.data for a in h), *(a.ctypes.data for a in sl), None, None, ids.ctypes.data,
                                            ids.size, ioff.ctypes.data, total.ctypes.data)
        assert rc == -1 and (ids == 0x5A5A5A5A).all() and (ioff == 0x5A5A5A5A).all() and (total == 0x5A5A5A5A).all(), word
        assert word in _lib.last_error(), (word, _lib.last_error())

    h = list(triples_csr(args["histories"], 3)); sl = list(triples_csr(args["selected"], 2))
    bump = lambda t, i, v: [np.concatenate([t[0][:i], [v], t[0][i + 1:]]).astype(np.int64)] + t[1:]
    raw(bump(h, 1, h[0][-1] + 5), sl, "hist_offsets")                                # decreasing
    raw(bump(h, 0, 1), sl, "hist_offsets")                                           # a first entry that is not 0
    raw(h, bump(sl, 1, sl[0][-1] + 5), "sel_offsets")
    raw(h, bump(sl, 0, 1), "sel_offsets")
    model.close()
    # an fp8 model
    from oracle import synth
    cfg8 = synth.make_config("f8t", mask_rate=0.2, mask_topk=4)
    cfg8["forward"] = "inference"
    m8 = ra.RecommenderModel(cfg8, dtype="fp8", max_rows=4)
    m8.load_state_dict(synth.make_params(cfg8, 5, "test"))
    a8 = serve.render_pack(states, pags, cfg8["max_sequence_length"], cfg8["vocab_sizes"]["0_matchedid"])
    untouched(m8, a8)
    from recommendersystem_amd import _lib
    assert "fp32 and bf16" in _lib.last_error()
    m8.close()
