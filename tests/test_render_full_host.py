"""CPU: the host side of rsys_render_request_full -- serve.render_pack(full_history=True) and the wave / row plan
(serve.render_full_plan, the statement of what the library runs) against a brute-force restatement."""
import numpy as np
import pytest

from recommendersystem_amd import serve

S, N0 = 16, 30
V = (30, 50)


def _user(rng, n_events):
    items, ts = [], 1.2e9
    for _ in range(n_events):
        ts += float(rng.integers(10, 10 ** 6))
        y = int(rng.integers(0, 2))
        items.append({"medium": y, "matchedid": int(rng.integers(1, V[y])), "history_max_ts": ts, "status": int(rng.integers(0, 9)),
                      "rating": float(rng.integers(0, 11)), "progress": float(rng.random()), "history_status": int(rng.integers(-1, 9)),
                      "history_rating": float(rng.integers(-1, 11))})
    return {"user": {"user": {"gender": [None, 0, 1][int(rng.integers(0, 3))], "source": int(rng.integers(0, 3))}, "items": items,
                     "timestamp": ts + 60.0}}


def _states(seed=3):
    rng = np.random.default_rng(seed)
    lens = [[0, 5], [3 * S], [S - 1, 1, 40]]
    states = [dict(medium=g % 2, items=[dict(medium=1, matchedid=7)] * (g == 1), users=[_user(rng, n) for n in ns],
                   penalties=dict(decay=0.9, mmr_penalty=0.1)) for g, ns in enumerate(lens)]
    return states, [{"offset": 0, "limit": 5}, {"offset": 5, "limit": 5}, {"offset": 0, "limit": 7}]


def test_pack_full_history():
    states, pags = _states()
    slots = {"0.retrieval": 0, "0.ranking": 1, "1.retrieval": 2, "1.ranking": 3}
    a = serve.render_pack(states, pags, S, N0, None, slots, full_history=True)
    users = [u["user"] for st in states for u in st["users"]]
    n = len(users)
    assert "ranking_prefix" not in a and "prefix_stride" not in a
    assert set(a) == {"group_medium", "offsets", "limits", "penalties", "group", "retrieval_rows", "retrieval_token", "user_desc", "user_ts",
                      "adapter_slots", "histories", "selected", "coef_have", "coefs"}
    assert a["user_desc"].shape == (n, 4) and a["user_desc"].dtype == np.int32
    assert a["retrieval_token"].shape == (n,) and a["retrieval_token"].dtype == np.int32 and a["user_ts"].dtype == np.float64
    assert all(a["retrieval_rows"][c].shape == (n, S) for c in serve._ROW_COLS)
    for i, u in enumerate(users):
        h = serve._history(u, S)
        assert a["user_desc"][i].tolist() == [len(h), 1, 0 if u["user"]["gender"] is None else u["user"]["gender"] + 1, u["user"]["source"]]
        assert a["retrieval_token"][i] == 2 * len(h) and a["user_ts"][i] == u["timestamp"]
        # columns [0, n_hist) of the retrieval row are the store row of predict_ranking_full; column n_hist is the query token
        d = serve._empty_rows(1, S)
        serve._fill_row(d, 0, h, len(h), u["user"], N0, False)
        for c in serve._ROW_COLS:
            assert np.array_equal(a["retrieval_rows"][c][i, :len(h)], d[c][0, :len(h)]), c
        assert a["retrieval_rows"]["matchedid"][i, len(h)] == -1 and a["retrieval_rows"]["rope_input_pos"][i, len(h)] == len(h)
    assert a["adapter_slots"] == [0, 1, 2, 3] and a["group"] == [0, 0, 1, 2, 2, 2]


def test_n_hist_is_the_length_of_the_kept_history():
    rng = np.random.default_rng(11)
    lens = [0, 1, S - 2, S - 1, S, 3 * S] + [int(x) for x in rng.integers(0, 4 * S, 20)]
    users = [_user(rng, n) for n in lens]
    states = [dict(medium=0, items=[], users=users)]
    a = serve.render_pack(states, {"offset": 0, "limit": 3}, S, N0, full_history=True)
    want = [len(serve._history(u["user"], S)) for u in users]
    assert a["user_desc"][:, 0].tolist() == want
    assert min(want) == 0 and max(want) == S - 1 and any(len(serve.project(serve.tokenize(u["user"]["items"]))) > S - 1 for u in users)


def test_pack_without_the_flag_is_unchanged():
    states, pags = _states(5)
    a = serve.render_pack(states, pags, S, N0)
    b = serve.render_pack(states, pags, S, N0, full_history=False)
    f = serve.render_pack(states, pags, S, N0, full_history=True)
    assert list(a) == list(b) == ["group_medium", "offsets", "limits", "penalties", "group", "retrieval_rows", "retrieval_token",
                                  "ranking_prefix", "prefix_stride", "user_desc", "user_ts", "adapter_slots", "histories", "selected",
                                  "coef_have", "coefs"]
    P = S // 2 - 1
    users = [u["user"] for st in states for u in st["users"]]
    assert a["prefix_stride"] == P and a["user_desc"][:, 0].tolist() == [min(P, len(serve._history(u, S))) for u in users]
    for k in a:
        if isinstance(a[k], dict):
            assert all(np.array_equal(a[k][c], b[k][c]) for c in a[k])
            if k == "retrieval_rows":
                assert all(np.array_equal(a[k][c], f[k][c]) for c in a[k])
        elif k not in ("adapter_slots",):
            assert np.array_equal(np.asarray(a[k], dtype=object if k in ("histories", "selected") else None),
                                  np.asarray(b[k], dtype=object if k in ("histories", "selected") else None)), k
    assert all(np.array_equal(a[k], f[k]) for k in ("retrieval_token", "user_ts", "penalties", "coefs", "coef_have"))
    assert np.array_equal(a["user_desc"][:, 1:], f["user_desc"][:, 1:])


def _brute(n_hist, n_cand, max_rows):
    """the forwards one after another, without serve's helpers: a list of ("store", [(user, slot, nh)]), ("cand", [(user, slot, first,
    count, nh)]) and ("empty", [(user, first, count)])"""
    out = []
    hist = [i for i in range(len(n_hist)) if n_hist[i] >= 1]
    while hist:
        wave, hist = hist[:max_rows], hist[max_rows:]
        out.append(("store", [(u, s, n_hist[u]) for s, u in enumerate(wave)]))
        rows = []
        for s, u in enumerate(wave):
            left, first = n_cand[u], 0
            while left > 0:
                rows.append((u, s, first, min(S, left), n_hist[u])); first += S; left -= S
        while rows:
            out.append(("cand", rows[:max_rows])); rows = rows[max_rows:]
    rows = []
    chunk = S - S // 2
    for u in range(len(n_hist)):
        if n_hist[u] == 0:
            left, first = n_cand[u], 0
            while left > 0:
                rows.append((u, first, min(chunk, left))); first += chunk; left -= chunk
    while rows:
        out.append(("empty", rows[:max_rows])); rows = rows[max_rows:]
    return out


@pytest.mark.parametrize("max_rows", [1, 2, 4])
def test_plan_against_brute_force(max_rows):
    cands = [1, S - 1, S, S + 1, 3 * S]
    n_hist = [3, 0, S - 1, 1, 0, 7, 2]
    for shift in range(len(cands)):
        n_cand = [cands[(i + shift) % len(cands)] for i in range(len(n_hist))]
        waves, empty = serve.render_full_plan(n_hist, n_cand, S, max_rows)
        got = []
        for store, batches in waves:
            got.append(("store", store))
            got += [("cand", b) for b in batches]
        got += [("empty", empty[r0:r0 + max_rows]) for r0 in range(0, len(empty), max_rows)]
        want = _brute(n_hist, n_cand, max_rows)
        assert got == want, (shift, got, want)
        counts = tuple(sum(1 for kind, _ in want if kind == k) for k in ("store", "cand", "empty"))
        assert serve.render_full_forwards(n_hist, n_cand, S, max_rows) == counts
        # every candidate of every user exactly once, in order
        seen = {u: [] for u in range(len(n_hist))}
        for kind, rows in want:
            for r in rows if kind != "store" else []:
                u, first, n = (r[0], r[2], r[3]) if kind == "cand" else r
                seen[u] += list(range(first, first + n))
        assert all(seen[u] == list(range(n_cand[u])) for u in seen)
    assert serve.render_full_plan([], [], S, max_rows) == ([], [])
