"""CPU: the host side of serve.render_users -- what it packs for rsys_render_request, with the model replaced by a recording
stand-in: retrieval rows and ranking prefixes against serve.build_batch, descriptors, the row plan per candidate count, the results'
shape for a page past the end."""
import numpy as np
import pytest

S, V = 16, (30, 40)
COLS = ("userid", "rope_input_pos", "token_mask_ids", "gender", "source", "matchedid", "status", "time", "rating", "progress")


def _user(rng, n_events, gender=None, source=2):
    items, ts = [], 1.2e9
    for _ in range(n_events):
        ts += float(rng.integers(10, 10 ** 6))
        y = int(rng.integers(0, 2))
        items.append({"medium": y, "matchedid": int(rng.integers(1, V[y])), "history_max_ts": ts, "status": int(rng.integers(0, 9)),
                      "rating": float(rng.integers(0, 11)), "progress": float(rng.random()), "history_status": -1, "history_rating": -1.0})
    return {"user": {"user": {"gender": gender, "source": source}, "items": items, "timestamp": ts + 60.0}}


def _states(rng):
    st = lambda m, users, items: dict(medium=m, items=items, users=users, penalties=dict(decay=0.9, mmr_penalty=0.2, related_penalty=0.3))
    return [st(1, [_user(rng, 5), _user(rng, 40, gender=1, source=0)], []),          # (40 events: longer than either row keeps)
            st(0, [_user(rng, 0)], [dict(medium=1, matchedid=7), dict(medium=0, matchedid=3)]),
            st(1, [_user(rng, 9, gender=0), _user(rng, 2), _user(rng, 12)], [dict(medium=1, matchedid=2)])]


class _Recorder:
    """stands in for RecommenderModel: records the one call and answers it"""
    max_rows = 4

    def __init__(self, answer, slots=None):
        self.config = {"max_sequence_length": S, "vocab_sizes": {"0_matchedid": V[0], "1_matchedid": V[1]}}
        self.calls = []
        self.answer = answer
        if slots:
            self.adapter_slots = slots

    def render_request(self, **kw):
        self.calls.append(kw)
        return self.answer


def test_render_users_packs_rows_prefixes_and_descriptors():
    from recommendersystem_amd import serve
    rng = np.random.default_rng(5)
    states = _states(rng)
    pags = [{"offset": 0, "limit": 10}, {"offset": 20, "limit": 7}, {"offset": 10 ** 6, "limit": 10}]
    registry = {"1.rating.coefs": np.array([0.3, 0.8]), "1.rating_mean": 4.0, "0.retrieval.coefs": np.array([0.5])}
    answer = ([np.arange(10, dtype=np.int32), np.arange(3, dtype=np.int32), np.zeros(0, np.int32)], np.array([33, 23, 17], np.int32))
    slots = {"0.retrieval": 0, "0.ranking": 1, "1.retrieval": 2, "1.ranking": 3}
    model = _Recorder(answer, slots)
    out = serve.render_users(model, states, pags, registry)
    assert len(model.calls) == 1                                              # ONE call for all states of both media
    a = model.calls[0]
    users = [(g, u["user"]) for g, st in enumerate(states) for u in st["users"]]
    assert a["group"] == [0, 0, 1, 2, 2, 2] and a["group_medium"] == [1, 0, 1]
    assert a["offsets"] == [0, 20, 10 ** 6] and a["limits"] == [10, 7, 10]
    assert np.array_equal(a["penalties"], np.array([[0.9, 0.2, 0.0, 0.3]] * 3, np.float32))
    assert a["adapter_slots"] == [0, 1, 2, 3]
    assert a["selected"] == [[], [(1, 7), (0, 3)], [(1, 2)]]
    assert a["histories"] == [[(x["medium"], x["matchedid"], x["status"]) for x in u["items"]] for _, u in users]
    assert a["coef_have"].tolist() == [1, 2]
    assert np.allclose(a["coefs"], [[0.5, 0, 0, 0], [0, 0.3, 0.8, 4.0]])
    P = a["prefix_stride"]
    assert P == S // 2 - 1
    nhs = []
    for i, (g, u) in enumerate(users):
        m = states[g]["medium"]
        # the retrieval row is the row of a one-user retrieval request
        d = serve.build_batch([u], "retrieval", m, V[0], S, 0)
        for c in COLS:
            assert a["retrieval_rows"][c][i].tobytes() == d[c][0].tobytes(), (c, i)
        index, _ = serve._selected_tokens([u], "retrieval", S, S)
        assert [int(a["retrieval_token"][i])] == index
        # the ranking prefix is the first nh columns of a ranking request's row, whatever its candidates
        nh = len(serve._history(u, S // 2))
        nhs.append(nh)
        d = serve.build_batch([dict(u, ranking_items=[1, 2, 3])], "ranking", m, V[0], S // 2, S - S // 2)
        for c in COLS:
            assert a["ranking_prefix"][c].shape == (len(users), P)
            assert a["ranking_prefix"][c][i, :nh].tobytes() == d[c][0, :nh].tobytes(), (c, i)
            assert not a["ranking_prefix"][c][i, nh:].any()
        who = u["user"]
        assert a["user_desc"][i].tolist() == [nh, 1, 0 if who["gender"] is None else who["gender"] + 1, who["source"]]
        assert a["user_ts"][i] == u["timestamp"]
    assert max(nhs) == P and min(nhs) == 0                                    # a clipped history and an empty one are both covered
    # results: the same [(page ids, total)] as serve.render; a page past the end is (empty, total)
    assert [(o[0].tolist(), o[1]) for o in out] == [(list(range(10)), 33), ([0, 1, 2], 23), ([], 17)]
    assert isinstance(out[2][1], int) and out[2][0].size == 0
    # a plain model: every row runs the base
    plain = _Recorder(answer)
    serve.render_users(plain, states, pags[0])                                # (one pagination for every state)
    assert plain.calls[0]["adapter_slots"] is None and plain.calls[0]["limits"] == [10, 10, 10]
    assert plain.calls[0]["coef_have"].tolist() == [0, 0]
    assert serve.render_users(plain, [], pags[0]) == [] and len(plain.calls) == 1


@pytest.mark.parametrize("S_", [16, 64, 1024])
def test_row_plan_chunks(S_):
    """`serve.render_row_plan` is the REFERENCE statement of the row plan, not the code that runs: the library plans the rows itself
    (model_render), and tests/test_gpu_render_request.py checks the rows it actually ran against this plan, at 1024 candidates
    too.  Here the reference is checked on its own terms -- descriptors and chunk counts for 0, 1, S - S // 2, S - S // 2 + 1 and 1024: every candidate in exactly one row,
    rows of at most S - S // 2 candidates that fit behind the longest history, action tokens as serve._selected_tokens gives them"""
    from recommendersystem_amd import serve
    chunk = S_ - S_ // 2
    for n, want_rows in ((0, 0), (1, 1), (chunk, 1), (chunk + 1, 2), (1024, -(-1024 // chunk))):
        for nh in (0, 3, S_ // 2 - 1):
            plan = serve.render_row_plan(n, nh, S_)
            assert len(plan) == want_rows
            assert [c0 for c0, _, _ in plan] == list(range(0, n, chunk))
            assert sum(k for _, k, _ in plan) == n and all(1 <= k <= chunk and nh + k <= S_ for _, k, _ in plan)
            for c0, k, tokens in plan:
                u = dict(items=[], ranking_items=list(range(k)))
                # (`_selected_tokens` recomputes nh from the history: give it one of nh distinct tokens)
                u["items"] = [{"medium": 0, "matchedid": j + 1, "history_max_ts": float(j), "status": 1, "rating": 1.0, "progress": 0.0,
                               "history_status": -1, "history_rating": -1.0} for j in range(nh)]
                index, counts = serve._selected_tokens([u], "ranking", S_, S_ // 2)
                assert tokens.tolist() == index and counts == [k]


def test_render_pack_rejects_bad_requests():
    from recommendersystem_amd import serve
    rng = np.random.default_rng(6)
    states = _states(rng)
    with pytest.raises(ValueError):
        serve.render_pack(states, {"offset": 0, "limit": 0}, S, V[0])
    with pytest.raises(ValueError):
        serve.render_pack(states, {"offset": -1, "limit": 5}, S, V[0])
    with pytest.raises(ValueError):
        serve.render_pack(states, [{"offset": 0, "limit": 5}], S, V[0])
    with pytest.raises(ValueError):
        serve.render_pack([dict(states[0], medium=2)], {"offset": 0, "limit": 5}, S, V[0])
    with pytest.raises(ValueError):
        serve.render_pack([dict(states[0], users=[])], {"offset": 0, "limit": 5}, S, V[0])


def test_wrapper_checks_shapes_before_the_library_is_called(monkeypatch):
    """RecommenderModel.render_request refuses arrays of the wrong size on the host"""
    from recommendersystem_amd import model as model_mod
    from recommendersystem_amd import serve
    rng = np.random.default_rng(7)
    states = _states(rng)
    args = serve.render_pack(states, {"offset": 0, "limit": 5}, S, V[0])

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")

    monkeypatch.setattr(model_mod, "lib", lambda: NoLib())
    m = model_mod.RecommenderModel.__new__(model_mod.RecommenderModel)
    m.config = {"max_sequence_length": S}
    m._h = None
    for bad in (dict(limits=[5, 5]), dict(user_ts=args["user_ts"][:-1]), dict(adapter_slots=[0, 1, 2]), dict(histories=args["histories"][:-1]),
                dict(selected=args["selected"][:-1]), dict(prefix_stride=args["prefix_stride"] + 1), dict(coefs=np.zeros(4, np.float32))):
        with pytest.raises(ValueError):
            m.render_request(**{**args, **bad})
