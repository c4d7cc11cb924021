"""CPU: the host side of serve.predict_ranking_full -- how users are packed into store waves and candidate rows, what
the rows hold, the order the outputs come back in, and the routing of users with an empty history -- on a recording stand-in for the
model, against a direct restatement."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _adapter_bank_util as ab  # noqa: E402


class FakeModel:
    """records the cache calls; a candidate's value = 1000 * slot's n_hist + its item id (so outputs name their slot and candidate)"""

    def __init__(self, S, V0, max_rows, slots=None):
        self.config = {"max_sequence_length": S, "vocab_sizes": {"0_matchedid": V0, "1_matchedid": V0}}
        self.max_rows = max_rows
        self.calls, self.cache = [], {}
        if slots:
            self.adapter_slots = slots

    def rank_cache_reserve(self, n):
        self.calls.append(("reserve", n)); self.rank_cache_slots = n

    def rank_cache_store(self, d, n_hist, slots, adapters=None):
        self.calls.append(("store", {k: v.copy() for k, v in d.items()}, list(n_hist), list(slots), adapters))
        for nh, s in zip(n_hist, slots):
            self.cache[s] = nh

    def rank_cache_candidates(self, d, slots, n_cand, adapters=None):
        self.calls.append(("cand", {k: v.copy() for k, v in d.items()}, list(slots), list(n_cand), adapters))
        return np.concatenate([1000.0 * self.cache[s] + d["matchedid"][r, :n] for r, (s, n) in enumerate(zip(slots, n_cand))]).astype(np.float32)

    def inference_select(self, d, task, index, adapters=None):
        self.calls.append(("select", d["matchedid"].shape[0], adapters))
        return -np.ones(len(index), np.float32)


def _users(rng, S, spec):
    out = []
    for nh, nc in spec:
        u = ab.make_user(rng, 0, [int(c) for c in rng.integers(1, 20, size=nc)])
        ts = 1.2e9
        for i in range(nh):                     # consecutive events on different items that change the state: nh projected tokens
            ts += 100.0
            u["items"].append({"medium": i % 2, "matchedid": 1 + i % 19, "history_max_ts": ts, "status": 1 + i % 5, "rating": float(i % 7),
                               "progress": 0.5, "history_status": -1, "history_rating": -1.0})
        u["timestamp"] = ts + 60.0
        out.append(u)
    return out


def test_plan_restated():
    from recommendersystem_amd import serve
    S, max_rows = 8, 2
    n_hist, n_cand = [3, 7, 1, 5, 2], [20, 1, 8, 9, 3]
    plan = serve.rank_cache_plan(n_hist, n_cand, S, max_rows)
    assert len(plan) == 3
    seen = {u: 0 for u in range(5)}
    for w, (store, batches) in enumerate(plan):
        users = list(range(2 * w, min(2 * w + 2, 5)))
        assert store == [(u, u - 2 * w, n_hist[u]) for u in users]
        rows = [r for b in batches for r in b]
        assert all(1 <= len(b) <= max_rows for b in batches)
        assert [r[0] for r in rows] == sorted(r[0] for r in rows)            # users in order, so the outputs are
        for u, slot, c0, n, pos in rows:
            assert slot == u - 2 * w and pos == n_hist[u] and c0 == seen[u] and 1 <= n <= S
            seen[u] += n
    assert seen == dict(enumerate(n_cand))
    assert sum(len(b) for _, bs in plan for b in bs) == sum(-(-c // S) for c in n_cand)


def test_rows_slots_positions_and_output_order():
    from recommendersystem_amd import serve
    S, V0 = 8, 100
    rng = np.random.default_rng(3)
    users = _users(rng, S, [(3, 20), (12, 1), (0, 4), (5, 9), (2, 0)])
    model = FakeModel(S, V0, max_rows=2, slots={"1.ranking": 3, "0.ranking": 1})
    out = serve.predict_ranking_full(model, users, 1)
    kept = [min(len(serve.project(serve.tokenize(u["items"]))), S - 1) for u in users]
    assert kept == [3, S - 1, 0, 5, 2]
    for u, nh, o in zip(users, kept, out):
        if nh == 0:
            assert o == {"1.ranking": [-1.0] * len(u["ranking_items"])}     # through predict (inference_select), untouched
        else:
            assert o == {"1.ranking": [1000.0 * nh + c + V0 for c in u["ranking_items"]]}
    kinds = [c[0] for c in model.calls]
    assert kinds[0] == "select" and model.calls[0][1:] == (1, [3])          # the empty history: one predict row with the ranking adapter
    assert kinds[1] == "reserve" and model.calls[1][1] >= 2
    stores = [c for c in model.calls if c[0] == "store"]
    assert [c[2] for c in stores] == [[3, S - 1], [5]] and [c[3] for c in stores] == [[0, 1], [0]] and all(c[4] == 3 for c in stores)
    # a history row = the first nh columns of build_batch's retrieval row (newest S - 1 events), nothing after them
    for c in stores:
        d = c[1]
        for row, nh in enumerate(c[2]):
            u = [users[0], users[1]][row] if c is stores[0] else users[3]
            want = serve.build_batch([u], "retrieval", 1, V0, S, 0)
            for k in d:
                assert np.array_equal(d[k][row, :nh], want[k][0, :nh]) and not d[k][row, nh:].any(), k
            assert np.array_equal(d["rope_input_pos"][row, :nh], np.arange(nh)) and not d["token_mask_ids"][row].any()
    cands = [c for c in model.calls if c[0] == "cand"]
    # user 0: 20 candidates = rows of 8, 8, 4; user 1: 1; wave of 2 rows each -> [u0, u0], [u0, u1]; then user 3: 8 + 1 -> [u3, u3]
    assert [c[2] for c in cands] == [[0, 0], [0, 1], [0, 0]] and [c[3] for c in cands] == [[8, 8], [4, 1], [8, 1]]
    assert all(c[4] == 3 for c in cands)
    first = cands[0][1]
    assert np.array_equal(first["matchedid"][0], np.array(users[0]["ranking_items"][:8]) + V0)
    assert np.array_equal(first["matchedid"][1], np.array(users[0]["ranking_items"][8:16]) + V0)
    assert (first["rope_input_pos"] == 3).all() and (cands[1][1]["rope_input_pos"][1] == S - 1).all()
    assert (first["status"] == -1).all() and not first["rating"].any() and (first["time"] == users[0]["timestamp"]).all()
    assert (cands[1][1]["matchedid"][1, 1:] == 0).all() and (cands[1][1]["userid"][1, 1:] == 0).all()     # padding behind the row's candidates
    # user 4 has a history and no candidates: nothing runs for it
    assert out[4] == {"1.ranking": []}


def test_empty_histories_only_never_touch_the_cache():
    from recommendersystem_amd import serve
    rng = np.random.default_rng(4)
    users = _users(rng, 8, [(0, 3), (0, 2)])
    model = FakeModel(8, 50, max_rows=4)
    out = serve.predict_ranking_full(model, users, 0)
    assert [c[0] for c in model.calls] == ["select", "select"] and all(c[1:] == (1, None) for c in model.calls)     # one row per user and chunk
    assert out == [{"0.ranking": [-1.0] * 3}, {"0.ranking": [-1.0] * 2}]


def test_empty_history_with_more_candidates_than_a_row():
    """an empty history and more than S candidates: one predict row per chunk of S - S // 2, as serve.render cuts them"""
    from recommendersystem_amd import serve
    rng = np.random.default_rng(6)
    S = 8
    users = _users(rng, S, [(0, 2 * S + 1), (0, S - 1)])
    model = FakeModel(S, 50, max_rows=4)
    out = serve.predict_ranking_full(model, users, 0)
    assert [c[0] for c in model.calls] == ["select"] * 7 and all(c[1:] == (1, None) for c in model.calls)     # 5 + 2 rows of <= 4 candidates
    assert out == [{"0.ranking": [-1.0] * (2 * S + 1)}, {"0.ranking": [-1.0] * (S - 1)}]
