"""GPU: rsys_render_request_full / serve.render_users(full_history=True) -- the one-call page pipeline with the ranking forward on
full-length histories through the per-user K/V cache.  The device's intermediates are read through the debug channel:
the store and candidate rows bit for bit against the rows serve.predict_ranking_full builds, the row records and forward counts against
serve.render_full_plan, the rating-head values against the float64 oracle on the reference's row and against the staged full-history
path, every downstream stage bit for bit given the device's own inputs.

Bounds.  fp32 against the staged path: rtol = atol = 1e-5, the bound the project uses for this forward (test_gpu_render_request).
bf16 against the staged path: twice the largest |difference| of serve.predict_ranking_full between a user run alone and the same user
at each position of a four-user call (S + 5 candidates, so every user spans two candidate rows).  That figure was measured on the commit
before this change, with this file's users (`_mixed_request`), on the bank model and on the plain model: BF16_PLACEMENT below.
`test_staged_full_history_placement` repeats the measurement on the staged path and asserts the recorded value."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_rank_np as rk  # noqa: E402
import _render_retrieval_np as rr  # noqa: E402
import test_gpu_rank_cache as trc  # noqa: E402
import test_gpu_render_request as trr  # noqa: E402
from test_gpu_rank_cache import make_user, oracle_full, relerr  # noqa: E402
from test_gpu_render_request import _render_user, _request, _tables  # noqa: E402

pytestmark = pytest.mark.gpu

COLS = trr.COLS
TASK_W = [0.05, 0.2, 0.3, 0.25]
# largest |difference| of serve.predict_ranking_full, one user alone vs inside a four-user call (see the header), per model kind
BF16_PLACEMENT = {"bank": 0.0, "base": 0.0}


def _model(name, kind, dtype, max_rows=4):
    cfg, V = trc._cfg(name)
    model, P, adapters = trc._model(cfg, kind, dtype, max_rows=max_rows)
    return cfg, V, model, P, adapters


def _wrap(user):
    """a request user of test_gpu_rank_cache.make_user as a state's user"""
    return {"user": {k: v for k, v in user.items() if k != "ranking_items"}}


def _mixed_request(seed=40):
    """the request of test_gpu_render_request (both media, 1-3 users per state, one history longer than a chunked row keeps, a page past
    the end) plus one user with an empty history and one with exactly S - 1 events"""
    cfg, V = trc._cfg("hd64")
    S = cfg["max_sequence_length"]
    states, pags, registry = _request(seed=seed)
    rng = np.random.default_rng(seed + 1000)
    states[0]["users"].append(_render_user(rng, V, 0))
    states[1]["users"].append(_wrap(make_user(rng, S - 1, [], V)))
    from recommendersystem_amd import serve
    lens = [len(serve._history(u["user"], S)) for st in states for u in st["users"]]
    assert 0 in lens and S - 1 in lens and (seed != 40 or any(S // 2 - 1 < n < S - 1 for n in lens)), lens
    return states, pags, registry


def _kept(model, cfg, states):
    S, D = cfg["max_sequence_length"], cfg["embed_dim"]
    g = model.render_kept
    k = {"forwards": g("forwards"), "full": g("forwards.full"), "queries": g("queries").reshape(-1, D), "counts": g("ret.counts"),
         "rows": g("rows").reshape(-1, 7), "groups": g("groups").reshape(-1, 6), "rm_users": g("rm_users").reshape(-1, 3),
         "r_masked": g("r_masked"), "r": g("r"), "picks": g("picks"), "store_rows": g("store.rows").reshape(-1, 4),
         "cand_tok": g("cand.token_index"), "tok": g("token_index")}
    k["ids"] = np.split(g("ret.ids"), np.cumsum(k["counts"])[:-1])
    for pre in ("store", "cand", "batch"):
        k[pre] = {c: g(f"{pre}.{c}").reshape(-1, S) for c in COLS}
    k["users"] = [(gi, u) for gi, st in enumerate(states) for u in st["users"]]
    return k


def _windows(k, states, pags, out):
    from recommendersystem_amd import serve
    active = {int(r[0]): r for r in k["groups"]}
    cand_of = {}
    for g, st in enumerate(states):
        assert out[g][1] == k["counts"][g]
        win = serve.page_window(int(k["counts"][g]), pags[g])
        if win is None:
            assert g not in active and out[g][0].size == 0
            continue
        cand_of[g] = k["ids"][g][win[0]:win[1]]
        assert (active[g][1], active[g][3], active[g][4], active[g][5]) == (int(st["medium"]), win[1] - win[0], win[2], win[3])
    return active, cand_of


def _plan_inputs(k, cfg, states, cand_of):
    """the users in r_masked order (medium 0's groups with a page, then medium 1's; user order inside) with their history and window sizes"""
    from recommendersystem_amd import serve
    S = cfg["max_sequence_length"]
    users = k["users"]
    order = [int(u) for u in k["rm_users"][:, 0]]
    assert order == [i for m in (0, 1) for i, (g, _) in enumerate(users) if int(states[g]["medium"]) == m and g in cand_of]
    hists = [serve._history(users[i][1]["user"], S) for i in order]
    return order, hists, [len(h) for h in hists], [int(cand_of[users[i][0]].size) for i in order]


def _check_assembly(model, cfg, V, states, pags, out, k):
    """test 1: store rows, candidate rows, positions, token indices, row records and forward counts"""
    from recommendersystem_amd import serve
    S, n0, RM = cfg["max_sequence_length"], V[0], model.max_rows
    users = k["users"]
    medium = [int(st["medium"]) for st in states]
    active, cand_of = _windows(k, states, pags, out)
    order, hists, nh, nc = _plan_inputs(k, cfg, states, cand_of)
    waves, empty = serve.render_full_plan(nh, nc, S, RM)
    assert k["full"].tolist() == list(serve.render_full_forwards(nh, nc, S, RM)), (k["full"], nh, nc)
    assert k["forwards"][1] == k["full"].sum() and k["forwards"][0] == -(-len(users) // RM)
    srow = crow = tok_at = rec_at = fwd = 0
    for w, (store, batches) in enumerate(waves):
        d = serve._empty_rows(len(store), S)
        for r, (i, slot, n) in enumerate(store):
            assert slot == r and n == nh[i] >= 1
            serve._fill_row(d, r, hists[i], n, users[order[i]][1]["user"]["user"], n0, False)
            assert k["store_rows"][srow + r].tolist() == [order[i], slot, n, w]
        for c in COLS:
            assert k["store"][c][srow:srow + len(store)].tobytes() == d[c].tobytes(), ("store", c, w)
        srow += len(store)
        for rows in batches:
            d = serve._empty_rows(len(rows), S)
            index = []
            for r, (i, slot, c0, n, h) in enumerate(rows):
                gi = order[i]
                g, u = users[gi][0], users[gi][1]["user"]
                seq = [serve.make_item(u["timestamp"], medium[g], int(c)) for c in cand_of[g][c0:c0 + n]]
                serve._fill_row(d, r, seq, 0, u["user"], n0, False)
                d["rope_input_pos"][r, :] = h
                index += [r * 2 * S + 2 * j + 1 for j in range(n)]
                assert k["rows"][rec_at].tolist() == [gi, g, int(active[g][2]) + c0, n, r, fwd, 0], (rec_at, k["rows"][rec_at])
                rec_at += 1
            for c in COLS:
                assert k["cand"][c][crow:crow + len(rows)].tobytes() == d[c].tobytes(), ("cand", c, fwd)
            assert k["cand_tok"][tok_at:tok_at + len(index)].tolist() == index
            tok_at += len(index); crow += len(rows); fwd += 1
    assert srow == k["store"]["time"].shape[0] == k["store_rows"].shape[0] and crow == k["cand"]["time"].shape[0]
    assert tok_at == k["cand_tok"].size
    brow = btok = 0
    for w0 in range(0, len(empty), RM):
        for r, (i, c0, n) in enumerate(empty[w0:w0 + RM]):
            gi = order[i]
            g, u = users[gi][0], users[gi][1]["user"]
            req = dict(u, ranking_items=[int(x) for x in cand_of[g][c0:c0 + n]])
            d = serve.build_batch([req], "ranking", medium[g], n0, S // 2, S - S // 2)
            for c in COLS:
                assert k["batch"][c][brow].tobytes() == d[c][0].tobytes(), ("batch", c, gi, c0)
            index, _ = serve._selected_tokens([req], "ranking", S, S // 2)
            assert (k["tok"][btok:btok + n] - r * 2 * S).tolist() == index
            assert k["rows"][rec_at].tolist() == [gi, g, int(active[g][2]) + c0, n, r, w0 // RM, 1]
            rec_at += 1; brow += 1; btok += n
    assert rec_at == k["rows"].shape[0] and brow == k["batch"]["time"].shape[0] and btok == k["tok"].size
    return active, cand_of


def _close(got, want, dtype, kind, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    diff = float(np.abs(got - want).max()) if got.size else 0.0
    print(f"{what} [{dtype} {kind}] max |diff| {diff:.3e}")
    if dtype == "fp32":
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
    elif BF16_PLACEMENT[kind] == 0.0:
        assert np.array_equal(got, want), (what, diff)
    else:
        assert diff <= 2.0 * BF16_PLACEMENT[kind], (what, diff, BF16_PLACEMENT[kind])


def _rm_of(k):
    return {int(u): k["r_masked"][int(o):int(o) + int(n)] for u, o, n in k["rm_users"]}


def _check_stages(model, cfg, V, related, states, pags, registry, dtype, kind, out, k, active, cand_of):
    """test 3: the two forwards against the staged full-history path, stage 6 bit for bit given the call's own r_masked"""
    from recommendersystem_amd import serve
    users = k["users"]
    group = np.array([g for g, _ in users], np.int32)
    medium = [int(st["medium"]) for st in states]
    want_q = [serve.predict(model, [u["user"]], "retrieval", medium[g])[0][f"{medium[g]}.retrieval"] for g, u in users]
    trr._close(k["queries"], want_q, dtype, "retrieval", "query buffer vs serve.predict")
    rm = _rm_of(k)
    for g in sorted(cand_of):
        m = medium[g]
        us = [i for i, (gg, _) in enumerate(users) if gg == g]
        reqs = [dict(users[i][1]["user"], ranking_items=[int(x) for x in cand_of[g]]) for i in us]
        for i, res in zip(us, serve.predict_ranking_full(model, reqs, m)):
            _close(rm[i], res[f"{m}.ranking"], dtype, kind, f"r_masked vs predict_ranking_full (user {i})")
    for m in (0, 1):
        gs = [g for g in sorted(cand_of) if medium[g] == m]
        if not gs:
            continue
        us = [i for i, (g, _) in enumerate(users) if g in gs]
        rc, kc, mean = serve._registry_coefs(registry, m)
        _, r = model.rank_request(k["queries"][us], m, [cand_of[g] for g in gs], group=[gs.index(group[i]) for i in us],
                                  r_masked=[rm[i] for i in us], retrieval_coef=rc, rating_coefs=kc, rating_mean=mean, rerank=False)
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


def _run(model, cfg, states, pags, registry, full=True):
    from recommendersystem_amd import serve
    model.render_keep(True)
    out = serve.render_users(model, states, pags, registry, full_history=full)
    return out, (_kept(model, cfg, states) if full else None)


# ---------------------------------------------------------------- 1. assembly, bit for bit
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_assembly_bit_for_bit(dtype):
    cfg, V, model, _, _ = _model("hd64", "bank", dtype)
    _tables(model, V)
    states, pags, registry = _mixed_request()
    out, k = _run(model, cfg, states, pags, registry)
    _check_assembly(model, cfg, V, states, pags, out, k)
    assert k["full"][0] >= 2 and k["full"][2] >= 1 and (k["rows"][:, 6] == 0).any() and (k["rows"][:, 6] == 1).any()
    assert out[3][0].size == 0 and not (k["rows"][:, 1] == 3).any()          # the page past the end: no ranking row
    model.close()


# ---------------------------------------------------------------- 2. the reference's function (the test that shows the function changed)
@pytest.mark.parametrize("kind", ["base", "bank"])
@pytest.mark.parametrize("name", ["tiny", "hd64"])
def test_full_pipeline_against_the_oracle(name, kind):
    """One user with S - 1 events, fp32: the kept r_masked of render_users(full_history=True) is within 1e-4 relative of the float64
    oracle on the reference's row (max_sequence_length = 2S, candidates in pieces of S), the bound of
    test_full_history_against_the_oracle; render_users without the flag, which ranks on S // 2 - 1 events, is more than 1e-2 away."""
    from recommendersystem_amd import serve
    cfg, V, model, P, adapters = _model(name, kind, "fp32")
    S = cfg["max_sequence_length"]
    _tables(model, V)
    rng = np.random.default_rng(5)
    medium = 1
    user = make_user(rng, S - 1, [], V)
    states = [dict(medium=medium, items=[], users=[_wrap(user)], penalties=dict(decay=0.9, mmr_penalty=0.1, same_series_penalty=0.5,
                                                                                  related_penalty=0.2))]
    pags = [{"offset": 0, "limit": 10}]
    out, k = _run(model, cfg, states, pags, None)
    cand = k["ids"][0][:serve.page_window(int(k["counts"][0]), pags[0])[1]]
    assert cand.size == k["r_masked"].size >= 1 and k["full"].tolist() == list(serve.render_full_forwards([S - 1], [cand.size], S, 4))
    assert k["rows"].shape[0] == -(-cand.size // S) and k["full"][0] == 1 and k["full"][2] == 0
    ref = np.concatenate([oracle_full(cfg, P, adapters, kind, dict(user, ranking_items=[int(c) for c in cand[c0:c0 + S]]), medium, V)
                          for c0 in range(0, cand.size, S)])
    old_out = serve.render_users(model, states, pags, None)
    old = model.render_kept("r_masked")
    assert np.array_equal(model.render_kept("ret.ids"), np.concatenate(k["ids"])) and old.size == ref.size
    e_new, e_old = relerr(k["r_masked"], ref), relerr(old, ref)
    print(f"one-call pipeline {name} {kind}: {cand.size} candidates, full-history err {e_new:.3e}, split row (S // 2 - 1 events) {e_old:.3e}")
    assert e_new < 1e-4, e_new
    assert e_old > 1e-2, e_old
    assert out[0][1] == old_out[0][1]
    model.close()


# ---------------------------------------------------------------- 3. stage parity with the staged full-history path
@pytest.mark.parametrize("kind", ["bank", "base"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stages_against_the_staged_full_history_path(kind, dtype):
    cfg, V, model, _, _ = _model("hd64", kind, dtype)
    related = _tables(model, V)
    states, pags, registry = _mixed_request()
    out, k = _run(model, cfg, states, pags, registry)
    active, cand_of = _check_assembly(model, cfg, V, states, pags, out, k)
    _check_stages(model, cfg, V, related, states, pags, registry, dtype, kind, out, k, active, cand_of)
    model.close()


def _placement_diff(model, cfg, V, states):
    """serve.predict_ranking_full for one user alone vs the same user at each position of a four-user call"""
    from recommendersystem_amd import serve
    S = cfg["max_sequence_length"]
    rng = np.random.default_rng(77)
    everyone = [u["user"] for st in states for u in st["users"]]
    with_hist = [u for u in everyone if serve._history(u, S)]
    worst = 0.0
    for st in states:
        m = int(st["medium"])
        cands = [int(x) for x in rng.choice(np.arange(1, V[m]), S + 5, replace=False)]
        others = [dict(with_hist[i % len(with_hist)], ranking_items=cands) for i in range(3)]
        for u in st["users"]:
            req = dict(u["user"], ranking_items=cands)
            one = np.asarray(serve.predict_ranking_full(model, [req], m)[0][f"{m}.ranking"], np.float32)
            for pos in range(4):
                four = serve.predict_ranking_full(model, others[:pos] + [req] + others[pos:], m)[pos][f"{m}.ranking"]
                worst = max(worst, float(np.abs(one - np.asarray(four, np.float32)).max()))
    print(f"one user vs a four-user call (staged full-history path): max |diff| {worst!r}")
    return worst


@pytest.mark.parametrize("kind", ["bank", "base"])
def test_staged_full_history_placement(kind):
    """the measurement behind the bf16 bound, on the staged path alone"""
    cfg, V, model, _, _ = _model("hd64", kind, "bf16")
    states, _, _ = _mixed_request()
    assert _placement_diff(model, cfg, V, states) == BF16_PLACEMENT[kind]
    model.close()


# ---------------------------------------------------------------- 4. the same function where both paths apply
def test_short_histories_equal_the_split_row_path():
    """fp32: users with at most S // 2 - 1 events (an empty history included) get the values of render_users without the flag within
    1e-5 relative (values, not pages: a near tie may reorder a page)"""
    from recommendersystem_amd import serve
    cfg, V, model, _, _ = _model("hd64", "bank", "fp32")
    S = cfg["max_sequence_length"]
    _tables(model, V)
    states, pags, registry = _mixed_request()
    short = [dict(st, users=[u for u in st["users"] if len(serve._history(u["user"], S)) <= S // 2 - 1]) for st in states]
    keep = [j for j, st in enumerate(short) if st["users"]]
    short, sp = [short[j] for j in keep], [pags[j] for j in keep]
    lens = [len(serve._history(u["user"], S)) for st in short for u in st["users"]]
    assert 0 in lens and max(lens) >= 2
    out, k = _run(model, cfg, short, sp, registry)
    serve.render_users(model, short, sp, registry)
    assert np.array_equal(model.render_kept("ret.ids"), np.concatenate(k["ids"]))
    old, old_users = model.render_kept("r_masked"), model.render_kept("rm_users").reshape(-1, 3)
    assert np.array_equal(old_users, k["rm_users"]) and old.size == k["r_masked"].size > 0
    for u, o, n in old_users:
        d = relerr(k["r_masked"][o:o + n], old[o:o + n])
        print(f"short history, user {u} ({lens[u]} events, {n} candidates): {d:.3e}")
        assert d < 1e-5, (u, d)
    model.close()


# ---------------------------------------------------------------- 5. waves
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_waves(dtype):
    states, pags, registry = _mixed_request()
    res = {}
    for max_rows in (32, 2):
        cfg, V, model, _, _ = _model("hd64", "bank", dtype, max_rows=max_rows)
        _tables(model, V)
        out, k = _run(model, cfg, states, pags, registry)
        _check_assembly(model, cfg, V, states, pags, out, k)
        res[max_rows] = k
        model.close()
    k2, k32 = res[2], res[32]
    n_cand_rows = int((k32["rows"][:, 6] == 0).sum())
    assert k2["full"][0] > 1 and k2["full"][1] > 1 and k2["full"][2] >= 1
    assert k32["full"].tolist()[:2] == [1, -(-n_cand_rows // 32)] and k32["forwards"][0] == 1
    assert np.array_equal(k2["counts"], k32["counts"]) and all(np.array_equal(a, b) for a, b in zip(k2["ids"], k32["ids"]))
    assert np.array_equal(k2["rm_users"], k32["rm_users"])
    _close(k2["r_masked"], k32["r_masked"], dtype, "bank", "r_masked, max_rows 2 vs 32")


# ---------------------------------------------------------------- 6. slot reuse
def test_slot_reuse():
    from recommendersystem_amd import serve
    cfg, V = trc._cfg("hd64")
    S = cfg["max_sequence_length"]
    rng = np.random.default_rng(61)
    pen = dict(decay=0.9, mmr_penalty=0.2, same_series_penalty=0.4, related_penalty=-0.3)
    mk = lambda lens, m: [dict(medium=m, items=[], penalties=pen, users=[_wrap(make_user(rng, n, [], V)) for n in lens])]
    calls = [mk([S - 1, 50, 40], 1), mk([5, 9, 3], 1), mk([17], 0)]         # long histories, shorter ones in the same slots, fewer users than slots
    pags = [{"offset": 0, "limit": 10}]

    def run(model, states):
        out, k = _run(model, cfg, states, pags, None)
        return out[0][0].tobytes(), out[0][1], k["r_masked"].tobytes(), k["full"].tolist()

    model, _, _ = trc._model(cfg, "bank", "fp32", max_rows=4)
    _tables(model, V)
    model.rank_cache_reserve(6)                                               # more slots than a wave uses: survives the calls
    other = make_user(rng, 21, rng.integers(1, V[0], size=7), V)
    dh, nh = trc._hist_rows(cfg, [other], V)
    model.rank_cache_store(dh, nh, [5])
    dc = trc._cand_rows(cfg, other, 0, V, [(0, 7)])
    before = model.rank_cache_candidates(dc, [5], [7])
    got = [run(model, st) for st in calls]
    assert model.rank_cache_slots == 6
    assert np.array_equal(before, model.rank_cache_candidates(dc, [5], [7]))  # an untouched slot answers as before
    model.close()
    for st, g in zip(calls, got):
        fresh, _, _ = trc._model(cfg, "bank", "fp32", max_rows=4)
        _tables(fresh, V)
        assert run(fresh, st) == g                                            # no stale K/V rows of an earlier user are read
        assert fresh.rank_cache_slots == 4
        fresh.close()
    assert got[0][3][0] == 1 and got[0][2] != got[1][2]


# ---------------------------------------------------------------- 7. a 1024-candidate slice
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_a_full_slice_of_1024_candidates(dtype):
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import serve
    cfg = trr._cfg()
    cfg["vocab_sizes"] = dict(cfg["vocab_sizes"], **{"1_matchedid": 1500})
    V = (cfg["vocab_sizes"]["0_matchedid"], 1500)
    S = cfg["max_sequence_length"]
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=4)
    model.load_state_dict(synth.make_params(cfg, 33, "test"))
    rng = np.random.default_rng(46)
    empty = lambda r, c: (np.zeros(c + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), (r, c))
    rel = {f"{m}.{k}": empty(V[m], V[1 - m] if k == "adaptations" else V[m]) for m in (0, 1) for k in serve.RELATION_KINDS}
    sim = {f"embeddings.{m}": (0.3 * rng.standard_normal((trr.DIM, V[m]))).astype(np.float32) for m in (0, 1)}
    related = {f"{m}.related": rr.random_csc(rng, V[m], V[m], 0.005) for m in (0, 1)}
    serve.load_retrieval_tables(model, rel, sim)
    serve.load_ranking_tables(model, related)
    states = [trr._state(rng, V, 1, 2, 0)]
    states[0]["users"][0] = _wrap(make_user(rng, S - 1, [], V))
    pags = [{"offset": 8, "limit": 8}]                                        # max_items_to_rank = 1024 - 1024 % 8 = 1024
    out, k = _run(model, cfg, states, pags, None)
    active, cand_of = _check_assembly(model, cfg, V, states, pags, out, k)
    _check_stages(model, cfg, V, related, states, pags, None, dtype, "base", out, k, active, cand_of)
    nh = [len(serve._history(u["user"], S)) for u in states[0]["users"]]
    want = serve.render_full_forwards(nh, [1024, 1024], S, 4)
    assert int(k["groups"][0][3]) == 1024 and out[0][0].size == 8
    assert k["rows"].shape[0] == sum(1024 // S if n else 1024 // (S - S // 2) for n in nh) and k["full"].tolist() == list(want)
    model.close()


# ---------------------------------------------------------------- 8. nothing else moves
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_request_between_training_steps_changes_nothing(dtype):
    """Deterministic mode: step -> load tables + render_users(full_history=True) -> step gives the step -> step results bit for bit."""
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
    states, pags, registry = _mixed_request(seed=44)

    def run(with_request):
        model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
        model.load_state_dict(P)
        opt = ra.create_optimizer(model, dict(cfg, learning_rate=1e-2))
        model.set_loss_weights(TASK_W, 1)
        out = []
        for i, (d, mk) in enumerate(zip(batches, masks)):
            if i == 1 and with_request:
                _tables(model, V)
                pages = serve.render_users(model, states, pags, registry, full_history=True)
                assert any(p[0].size for p in pages) and model.render_kept("forwards.full")[0] >= 1
            out.append(np.array(model(d, False, masks=mk), np.float32))
            out += [model.grad(n).copy() for n in names]
            opt.step(clip_max_norm=1.0)
        out += [model.get_parameter(n).copy() for n in names]
        model.close()
        return out

    a, b = run(False), run(True)
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_reproducible():
    cfg, V, model, _, _ = _model("hd64", "bank", "bf16")
    _tables(model, V)
    states, pags, registry = _mixed_request(seed=43)
    keys = ["queries", "ret.ids", "ret.counts", "r_masked", "r", "picks", "cand.token_index", "cand.matchedid", "store.time", "rows", "groups"]
    res = []
    for _ in range(2):
        out, _ = _run(model, cfg, states, pags, registry)
        res.append(([model.render_kept(x).tobytes() for x in keys], [(o[0].tobytes(), o[1]) for o in out]))
    assert res[0] == res[1]
    model.close()


# ---------------------------------------------------------------- 9. the assembly's column loop past one workgroup's width
def test_assembly_past_one_workgroup_of_columns():
    """S = 320: more columns than the 256 threads of a row's workgroup and no multiple of them, so the assembly kernel's column loop takes
    a second, partial step.  Past column 256 it copies history columns only in the store rows of rsys_render_request_full (n_hist = 319);
    a split row's prefix holds at most S // 2 - 1 = 159 columns and the windows here hold fewer than 97 candidates, so in
    rsys_render_request, and in the candidate rows, the second step writes the zero columns behind the candidates.  One state per
    medium, each with a user of more than S events (n_hist = S - 1: more than 256 history columns are copied), one of 10 events and one
    of none; fp32, base model, max_rows 4.  Both entry points: the store, candidate and batch rows and the token indices bit for bit
    against serve._fill_row / build_batch (`_check_assembly`, test_gpu_render_request._check_request)."""
    from oracle import synth
    from recommendersystem_amd import serve
    cfg = synth.make_config("hd64", mask_rate=0.2, mask_topk=4, max_sequence_length=320)
    cfg["forward"] = "inference"
    cfg["vocab_sizes"] = dict(cfg["vocab_sizes"], **{"0_matchedid": 400, "1_matchedid": 600})   # (candidates are left beside 319 events)
    V = (400, 600)
    S = cfg["max_sequence_length"]
    assert S > 256 and S % 256
    model, _, _ = trc._model(cfg, "base", "fp32", max_rows=4)
    related = _tables(model, V)
    rng = np.random.default_rng(91)
    pen = dict(decay=0.9, mmr_penalty=0.2, same_series_penalty=0.4, related_penalty=-0.3)
    states = [dict(medium=m, items=[], penalties=pen, users=[_wrap(make_user(rng, n, [], V)) for n in (S + 20, 10, 0)]) for m in (0, 1)]
    assert [len(serve._history(u["user"], S)) for st in states for u in st["users"]] == [S - 1, 10, 0] * 2
    pags = [{"offset": 0, "limit": 10}] * 2
    out, k = _run(model, cfg, states, pags, None)
    _check_assembly(model, cfg, V, states, pags, out, k)
    assert k["store_rows"][:, 2].max() == S - 1 > 256                                           # history columns past 256 are copied
    assert (k["rows"][:, 6] == 0).any() and (k["rows"][:, 6] == 1).any()
    out = serve.render_users(model, states, pags, None)
    ks = trr._check_request(model, cfg, V, related, states, pags, None, "fp32", out)
    assert ks["rows"].shape[0] >= 6 and ks["batch"]["time"].shape == (ks["rows"].shape[0], S)
    model.close()


# ---------------------------------------------------------------- 10. errors leave the outputs untouched
def _raw(model, args, ids_cap=None):
    """rsys_render_request_full on sentinel-filled outputs: (return code, outputs untouched)"""
    from recommendersystem_amd import _lib
    from recommendersystem_amd.model import triples_csr
    S = model.config["max_sequence_length"]
    gm = np.asarray(args["group_medium"], np.int32); off = np.asarray(args["offsets"], np.int64); lim = np.asarray(args["limits"], np.int32)
    pen = np.ascontiguousarray(args["penalties"], np.float32); gp = np.asarray(args["group"], np.int32)
    ng, nu = gm.size, gp.size
    rb, keep_r = model._c_rows(args["retrieval_rows"], nu, S)
    tok = np.asarray(args["retrieval_token"], np.int32); desc = np.ascontiguousarray(args["user_desc"], np.int32)
    ts = np.asarray(args["user_ts"], np.float64)
    sl = None if args["adapter_slots"] is None else np.asarray(args["adapter_slots"], np.int32)
    h = triples_csr(args["histories"], 3); sel = triples_csr(args["selected"], 2)
    ch = np.asarray(args["coef_have"], np.int32); cf = np.ascontiguousarray(args["coefs"], np.float32)
    cap = int(lim.sum()) if ids_cap is None else ids_cap
    ids = np.full(int(lim.sum()), 0x5A5A5A5A, np.int32); ioff = np.full(ng + 1, 0x5A5A5A5A, np.int64); total = np.full(ng, 0x5A5A5A5A, np.int32)
    rc = _lib.lib().rsys_render_request_full(model._h, ng, gm.ctypes.data, off.ctypes.data, lim.ctypes.data, pen.ctypes.data, nu, gp.ctypes.data,
                                             C.byref(rb), tok.ctypes.data, desc.ctypes.data, ts.ctypes.data,
                                             None if sl is None else sl.ctypes.data, *(a.ctypes.data for a in h),
                                             *(a.ctypes.data for a in sel), ch.ctypes.data, cf.ctypes.data, ids.ctypes.data, cap,
                                             ioff.ctypes.data, total.ctypes.data)
    return rc, bool((ids == 0x5A5A5A5A).all() and (ioff == 0x5A5A5A5A).all() and (total == 0x5A5A5A5A).all())


def test_errors_leave_the_outputs_untouched():
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import _lib, serve
    cfg, V, model, _, _ = _model("hd64", "bank", "fp32")
    S = cfg["max_sequence_length"]
    _tables(model, V)
    states, pags, registry = _mixed_request(seed=45)
    args = serve.render_pack(states, pags, S, V[0], registry, model.adapter_slots, full_history=True)
    assert _raw(model, args) == (0, False)
    nu = len(args["group"])

    def bad(word, **kw):
        assert _raw(model, {**args, **{k: v for k, v in kw.items() if k != "ids_cap"}}, kw.get("ids_cap")) == (-1, True), word
        assert word in _lib.last_error(), (word, _lib.last_error())

    desc = args["user_desc"].copy(); desc[0, 0] = S
    bad("n_hist", user_desc=desc)                                              # n_hist = S
    desc = args["user_desc"].copy(); desc[1, 0] = -1
    bad("n_hist", user_desc=desc)                                              # n_hist negative
    bad("every group needs", group=[0] * nu)                                   # a group without users
    bad("ids_out", ids_cap=int(np.sum(args["limits"])) - 1)                    # ids_cap too small
    bad("adapter slot", adapter_slots=[0, 1, 2, 6])                            # a slot that was never loaded
    model.clear_adapter(3)
    bad("adapter slot")                                                        # an incomplete adapter slot ("1.ranking")
    with pytest.raises(ra.RsysError):
        model.render_request_full(**args)
    model.close()
    for kind in ("fp8", "sharded"):
        if kind == "fp8":
            c8 = synth.make_config("f8t", mask_rate=0.2, mask_topk=4)
            c8["forward"] = "inference"
            m8 = ra.RecommenderModel(c8, dtype="fp8", max_rows=4)
        else:
            c8 = synth.make_config("tiny", mask_rate=0.2, mask_topk=4)
            c8["forward"] = "inference"
            c8["table_shard"] = (0, 1)
            m8 = ra.RecommenderModel(c8, dtype="fp32", max_rows=4)
        a8 = serve.render_pack(states, pags, c8["max_sequence_length"], c8["vocab_sizes"]["0_matchedid"], full_history=True)
        assert _raw(m8, a8) == (-1, True), kind
        assert ("fp32 and bf16" if kind == "fp8" else "replicated") in _lib.last_error()
        m8.close()
