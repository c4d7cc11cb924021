"""CPU: the host side of weighted multi-query states (rsys_query_weights_set) -- the float32 twin against the unweighted
restatements at weight one, the zero-weight rule, and the array builders of serve.py."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _query_weights_np as qw  # noqa: E402
import _render_retrieval_np as rr  # noqa: E402

V = (90, 70)
DIM = 8


def _sim(rng):
    sim = {f"embeddings.{m}": rng.standard_normal((DIM, V[m])).astype(np.float32) for m in (0, 1)}
    sim.update({f"crossproject.{m}": rng.standard_normal((DIM, DIM)).astype(np.float32) for m in (0, 1)})
    return sim


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_weight_one_is_the_unweighted_restatement(seed):
    rng = np.random.default_rng(seed)
    rel = rr.random_relations(rng, V)
    sim = _sim(rng)
    for m in (0, 1):
        st = rr.random_state(rng, V, m, n_users=3, n_items=12, n_selected=3)
        logp = [rng.standard_normal(V[m]).astype(np.float32) for _ in st["users"]]
        # today's sum: p += log p_u in user order, on top of a prior
        prior = rng.standard_normal(V[m]).astype(np.float32)
        p = prior.copy()
        for row in logp:
            p = (p + row).astype(np.float32)
        want, adm = rr.literal(m, rel, st, V, p=p)
        for weights in (None, 1.0):
            s1 = copy.deepcopy(st)
            if weights is not None:
                for e in s1["users"] + s1["items"]:
                    e["weight"] = weights
            got, adm1 = qw.literal_weighted(m, rel, s1, V, logp=logp, prior=prior)
            assert got.tobytes() == want.tobytes() and np.array_equal(adm, adm1)
        # the prior: E' (sum of x_a) at weight one, the device's association (rsys_retrieve_request)
        rows = []
        for a in st["items"]:
            x = sim[f"embeddings.{a['medium']}"][:, a["matchedid"]]
            rows.append(x if a["medium"] == m else sim[f"crossproject.{a['medium']}"] @ x)
        s = np.zeros(DIM, np.float32)
        for x in rows:
            s = (s + x).astype(np.float32)
        assert qw.prior_weighted(m, sim, st, V).tobytes() == (sim[f"embeddings.{m}"].T @ s).astype(np.float32).tobytes()
        # ranking: the unweighted sum over users
        terms = [rng.standard_normal(17).astype(np.float32) for _ in st["users"]]
        r = np.zeros(17, np.float32)
        for t in terms:
            r = (r + t).astype(np.float32)
        assert qw.ranking_weighted(st, terms).tobytes() == r.tobytes()


def test_masks_ignore_weights_and_zero_skips_the_term():
    rng = np.random.default_rng(5)
    rel = rr.random_relations(rng, V)
    st = rr.random_state(rng, V, 0, n_users=3, n_items=12, n_selected=2)
    logp = [rng.standard_normal(V[0]).astype(np.float32) for _ in st["users"]]
    logp[1][7] = -np.inf
    logp[1][9] = np.nan
    _, adm = qw.literal_weighted(0, rel, st, V, logp=logp)
    for z in (0.0, -0.0):
        s0 = copy.deepcopy(st)
        s0["users"][1]["weight"] = z
        s0["users"][2]["weight"] = -1.5
        p, adm0 = qw.literal_weighted(0, rel, s0, V, logp=logp)
        # the masks are those of the state with every user, whatever the weights; the zero-weight user's -inf / NaN never enter the sum
        free = [i for i in (7, 9) if adm[i]]
        assert all(np.isfinite(p[i]) for i in free)
        assert np.array_equal(adm0[np.isfinite(logp[1])], adm[np.isfinite(logp[1])])
        want = qw.fadd(logp[0], qw.fmul(np.float32(-1.5), logp[2]))
        assert p[adm0].tobytes() == want[adm0].tobytes()
    # a running sum of -0.0 keeps its sign bit under a zero weight
    assert np.signbit(qw.weighted_add(np.float32(-0.0), 0.0, np.float32(3.0)))
    assert qw.weighted_add(np.float32(2.0), -0.0, np.float32(np.nan)) == 2.0


def _states(histories=True):
    """three states over both media; histories=False: users without list items (render_pack tokenises full history records)"""
    rng = np.random.default_rng(3)
    states = []
    for m, nu, ns in ((0, 2, 1), (1, 1, 2), (0, 3, 0)):
        st = rr.random_state(rng, V, m, n_users=nu, n_items=5, n_selected=ns)
        for u in st["users"]:
            u["embeds"] = {f"{m}.retrieval": rng.standard_normal(4).astype(np.float32), f"{m}.ranking": np.zeros(2, np.float32)}
            u["user"].update(user=dict(gender=None, source=0), timestamp=1.3e9)
            if not histories:
                u["user"]["items"] = []
        states.append(st)
    return states


def test_builders_emit_weights_in_user_and_item_order():
    from recommendersystem_amd import serve
    states = _states()
    med0 = [states[0], states[2]]
    # no "weight" key anywhere: no weight arrays, and the tuples keep their shape without weights=True
    assert serve.state_weights(states) == (None, None)
    assert len(serve.request_arrays(med0, 0)) == 4 and len(serve._window_arrays(med0, 0)) == 4
    assert len(serve.rank_arrays(med0, [[1, 2], [3, 4]])) == 5
    assert serve.request_arrays(med0, 0, weights=True)[4:] == (None, None)
    states[0]["users"][1]["weight"] = 0.25
    states[2]["users"][0]["weight"] = -2.0
    states[1]["items"][1]["weight"] = 0.0
    uw, sw = serve.request_arrays(med0, 0, weights=True)[4:]
    assert uw.dtype == np.float32 and uw.tolist() == [1.0, 0.25, -2.0, 1.0, 1.0] and sw is None      # (medium 0 has no weighted item)
    uw, sw = serve._window_arrays([states[1]], 1, weights=True)[4:]
    assert uw is None and sw.dtype == np.float32 and sw.tolist() == [1.0, 0.0]
    assert serve.rank_arrays(med0, [[1, 2], [3, 4]], weights=True)[5].tolist() == [1.0, 0.25, -2.0, 1.0, 1.0]
    uw, sw = serve.state_weights(states)
    assert uw.tolist() == [1.0, 0.25, 1.0, -2.0, 1.0, 1.0] and sw.tolist() == [1.0, 1.0, 0.0]
    # a state without an "items" key (what `ranking` may be handed) has no selected items
    assert serve.state_weights([dict(medium=0, users=[{"weight": 2.0}])])[0].tolist() == [2.0]
    assert serve.state_weights([dict(medium=0, users=[{}])]) == (None, None)


def test_render_pack_carries_weights_only_when_a_state_has_them():
    from recommendersystem_amd import serve
    states = _states(histories=False)
    a = serve.render_pack(states, {"offset": 0, "limit": 5}, 16, V[0])
    assert "user_weights" not in a and "selected_weights" not in a
    states[1]["users"][0]["weight"] = 3.0
    a = serve.render_pack(states, {"offset": 0, "limit": 5}, 16, V[0], full_history=True)
    assert a["user_weights"].tolist() == [1.0, 1.0, 3.0, 1.0, 1.0, 1.0] and a["selected_weights"] is None
    states[0]["items"][0]["weight"] = -1.0
    a = serve.render_pack(states, {"offset": 0, "limit": 5}, 16, V[0])
    assert a["selected_weights"].tolist() == [-1.0, 1.0, 1.0]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_weight_raises(bad):
    from recommendersystem_amd import serve
    from recommendersystem_amd.model import query_weights_array
    states = _states(histories=False)
    states[0]["users"][0]["weight"] = bad
    with pytest.raises(ValueError):
        serve.state_weights(states)
    with pytest.raises(ValueError):
        serve.request_arrays([states[0]], 0, weights=True)
    with pytest.raises(ValueError):
        query_weights_array([1.0, bad])
    del states[0]["users"][0]["weight"]
    states[1]["items"][0]["weight"] = bad
    with pytest.raises(ValueError):
        serve.render_pack(states, {"offset": 0, "limit": 5}, 16, V[0])
