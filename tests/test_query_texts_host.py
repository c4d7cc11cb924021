"""CPU: the host side of text queries in request states (rsys_query_texts_set) -- the builder `serve.state_texts`, the
float32 twin tests/_query_texts_np.py against the existing twins where no text is given, and the argument rules of the setter that need
no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _query_texts_np as qt  # noqa: E402
import _query_weights_np as qw  # noqa: E402

Q = 6


def _states(rng):
    """four states over both media; states 0 and 3 hold texts, state 1 an empty list, state 2 no key"""
    emb = lambda: rng.standard_normal(Q).astype(np.float32)
    return [dict(medium=1, users=[], items=[], texts=[{"embedding": emb()}, {"embedding": emb(), "weight": -0.5}]),
            dict(medium=0, users=[], items=[], texts=[]),
            dict(medium=0, users=[], items=[]),
            dict(medium=0, users=[], items=[], texts=[{"embedding": emb(), "weight": 0.0}])]


def test_state_texts_defaults_and_order():
    from recommendersystem_amd import serve
    rng = np.random.default_rng(0)
    states = _states(rng)
    x, group, w = serve.state_texts(states)
    assert x.dtype == np.float32 and x.shape == (3, Q) and group.dtype == np.int32 and group.tolist() == [0, 0, 3]
    assert w.dtype == np.float32 and w.tolist() == [1.0, -0.5, 0.0] and np.signbit(w).tolist() == [False, True, False]
    want = [t["embedding"] for st in states for t in st.get("texts", ())]
    assert x.tobytes() == np.stack(want).tobytes()
    # per medium: groups stay indices into the list handed in
    x1, g1, w1 = serve.state_texts(states, 1)
    assert g1.tolist() == [0, 0] and w1.tolist() == [1.0, -0.5]
    x0, g0, w0 = serve.state_texts(states, 0)
    assert g0.tolist() == [3] and w0.tolist() == [0.0] and x0.tobytes() == x[2:].tobytes()
    # no "weight" key anywhere: weights is None; no text anywhere: None, the setter is not called
    del states[0]["texts"][1]["weight"]
    assert serve.state_texts(states, 1)[2] is None
    assert serve.state_texts(states[1:3]) is None and serve.state_texts([]) is None
    assert serve.state_texts([states[0]], 0) is None


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_texts_raise(bad):
    from recommendersystem_amd import serve
    states = _states(np.random.default_rng(1))
    states[0]["texts"][0]["weight"] = bad
    with pytest.raises(ValueError):
        serve.state_texts(states)
    del states[0]["texts"][0]["weight"]
    states[3]["texts"][0]["embedding"][2] = bad
    with pytest.raises(ValueError):
        serve.state_texts(states)
    states[3]["texts"][0]["embedding"] = np.zeros(Q + 1, np.float32)      # two widths in one request
    with pytest.raises(ValueError):
        serve.state_texts(states)


class _Recorder:
    def __init__(self):
        self.calls = []

    def query_texts_set(self, search_model, medium, x, group, weights=None):
        if search_model == "fails":
            raise RuntimeError("the library refused the set")
        self.calls.append((search_model, medium, x, group, weights))


def test_the_setter_is_called_per_medium_and_only_for_states_with_texts():
    from recommendersystem_amd import serve
    states = _states(np.random.default_rng(2))
    rec = _Recorder()
    serve._texts_before(rec, states[1:3], None)                 # no texts: nothing is called, no `search` is needed
    assert rec.calls == []
    serve._texts_before(rec, states, {0: "s0", 1: "s1"})
    assert [(c[0], c[1], c[3].tolist()) for c in rec.calls] == [("s0", 0, [3]), ("s1", 1, [0, 0])]
    assert rec.calls[0][4].tolist() == [0.0] and rec.calls[1][4].tolist() == [1.0, -0.5]
    # a medium with texts and no `search` entry raises before the first setter call: nothing is left pending on the model
    for search in (None, {}, {0: "s0"}, {1: "s1"}):
        rec = _Recorder()
        with pytest.raises(ValueError):
            serve._texts_before(rec, states, search)
        assert rec.calls == []
    # the second medium's set fails: the first one's is cleared (n = 0)
    rec = _Recorder()
    with pytest.raises(RuntimeError):
        serve._texts_before(rec, states, {0: "s0", 1: "fails"})
    assert [(c[0], c[1], c[2].shape[0]) for c in rec.calls] == [("s0", 0, 1), (None, 0, 0)]
    # the request's wrapper raises after the sets were made: both are cleared; a request that returns clears nothing
    rec = _Recorder()
    with pytest.raises(KeyError):
        with serve._texts(rec, states, {0: "s0", 1: "s1"}):
            raise KeyError("a check of the wrapper")
    assert [(c[0], c[1], c[2].shape[0]) for c in rec.calls] == [("s0", 0, 1), ("s1", 1, 2), (None, 0, 0), (None, 1, 0)]
    rec = _Recorder()
    with serve._texts(rec, states, {0: "s0", 1: "s1"}):
        pass
    assert [c[1] for c in rec.calls] == [0, 1]


def test_twin_without_texts_is_the_existing_twin():
    rng = np.random.default_rng(3)
    V, n = 40, 9
    prior = rng.standard_normal(V).astype(np.float32)
    rows = [rng.standard_normal(V).astype(np.float32) for _ in range(3)]
    none_z, none_lse = np.zeros((0, V), np.float32), np.zeros(0, np.float32)
    for uw in (None, [0.5, -1.0, 0.0]):
        want = qw.chain(prior, rows, [1.0] * 3 if uw is None else uw)
        assert qt.retrieval(prior, none_z, none_lse, None, rows, uw).tobytes() == want.tobytes()
    assert qt.userless(prior, none_z, none_lse).tobytes() == prior.tobytes()
    cand = rng.choice(V, n, replace=False)
    terms = [rng.standard_normal(n).astype(np.float32) for _ in range(3)]
    st = dict(users=[{"weight": 0.5}, {}, {"weight": -2.0}])
    assert qt.ranking(none_z, none_lse, cand, None, terms, qw.user_weights(st)).tobytes() == qw.ranking_weighted(st, terms).tobytes()
    r = np.zeros(n, np.float32)
    for t in terms:
        r = (r + t).astype(np.float32)
    assert qt.ranking(none_z, none_lse, cand, None, terms).tobytes() == r.tobytes()


def test_twin_chains():
    rng = np.random.default_rng(4)
    V = 33
    z = rng.standard_normal((2, V)).astype(np.float32) * 5
    lse = np.array([7.25, 3.5], np.float32)
    z[1, 4] = -np.inf
    prior = rng.standard_normal(V).astype(np.float32)
    rows = [rng.standard_normal(V).astype(np.float32)]
    # one rounding per operation, text order, then the users
    s = prior.copy()
    for t, w in ((0, 0.5), (1, -1.0)):
        s = (s + (np.float32(w) * (z[t] - lse[t]).astype(np.float32)).astype(np.float32)).astype(np.float32)
    s = (s + rows[0]).astype(np.float32)
    got = qt.retrieval(prior, z, lse, [0.5, -1.0], rows)
    assert got.tobytes() == s.tobytes() and got[4] == np.inf
    # a zero weight skips the text, whatever it holds: every bit of the request without it
    for zero in (0.0, -0.0):
        assert qt.retrieval(prior, z, lse, [0.5, zero], rows).tobytes() == qt.retrieval(prior, z[:1], lse[:1], [0.5], rows).tobytes()
        assert qt.userless(prior, z, lse, [zero, zero]).tobytes() == prior.tobytes()
    # ranking starts from +0.0 and gathers the candidates
    cand = np.array([4, 0, 32, 7])
    r = qt.ranking(z, lse, cand, [1.0, 0.0])
    assert r.tobytes() == (np.float32(0.0) + (z[0, cand] - lse[0]).astype(np.float32)).astype(np.float32).tobytes()
    assert not np.signbit(qt.ranking(z, lse, cand, [0.0, -0.0])).any()


def test_setter_argument_rules_without_a_device():
    import recommendersystem_amd as ra
    from recommendersystem_amd._lib import lib
    L = lib()
    x = np.zeros((2, Q), np.float32)
    g = np.zeros(2, np.int32)
    out = np.full(2, -7, np.int64)
    assert L.rsys_query_texts_set(None, None, 0, x.ctypes.data, 2, g.ctypes.data, None) == -1          # a null model handle
    assert L.rsys_query_texts_pending(None, out.ctypes.data) == -1 and (out == -7).all()
    assert L.rsys_op_text_rows(None, x.ctypes.data, 2, x.ctypes.data, x.ctypes.data) == -1             # a null search handle
    # the method's own checks come before the library is reached (no handle is read)
    set_texts = ra.RecommenderModel.query_texts_set
    with pytest.raises(ValueError):
        set_texts(object(), None, 0, x, [0])                         # one group for two texts
    with pytest.raises(ValueError):
        set_texts(object(), None, 0, x, [0, 0], [1.0])               # one weight for two texts
    with pytest.raises(ValueError):
        set_texts(object(), None, 0, x, [0, 0], [1.0, np.nan])       # a non-finite weight
