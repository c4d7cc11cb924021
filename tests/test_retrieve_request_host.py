"""CPU: the render.jl `retrieval(state)` restatement in its two forms (tests/_render_retrieval_np.py) and the host side of
rsys_retrieve_request -- how serve.retrieval packs render.jl states into the CSR arrays of the C call, and how load_retrieval_tables
reads render.jl's tables.  No GPU: the C entry point is replaced by a recorder."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_retrieval_np as rr  # noqa: E402


@pytest.mark.parametrize("seed", range(12))
def test_literal_and_set_forms_agree(seed):
    rng = np.random.default_rng(seed)
    V = (int(rng.integers(20, 90)), int(rng.integers(20, 90)))
    rel = rr.random_relations(rng, V, density=float(rng.choice([0.01, 0.05, 0.15])))
    for m in (0, 1):
        st = rr.random_state(rng, V, m, n_users=int(rng.integers(1, 4)), n_items=40, n_selected=int(rng.integers(0, 4)))
        released = rng.random(V[m]) < 0.8 if seed % 2 else None
        _, adm = rr.literal(m, rel, st, V, released=released)
        masked = rr.set_mask(m, rel, st, V, released=released)
        assert np.array_equal(adm, ~masked)


def test_restatement_cases_cover_the_rules():
    """the random cases above reach every rule: each alone masks something on some seed"""
    hits = dict(adapt=0, recap=0, missing_dep=0, sequel=0, dup=0, zeros=0)
    for seed in range(12):
        rng = np.random.default_rng(seed)
        V = (60, 60)
        rel = rr.random_relations(rng, V, density=0.05)
        hits["zeros"] += int((rel["0.dependencies"][2] == 0).sum())
        st = rr.random_state(rng, V, 0, 2, 40, 2)
        for u in st["users"]:
            keys = [(x["medium"], x["matchedid"]) for x in u["user"]["items"]]
            hits["dup"] += len(keys) - len(set(keys))
        dep, rec, ada = (rel[f"0.{k}"] for k in ("dependencies", "recaps", "adaptations"))
        for u in st["users"]:
            last = {(x["medium"], x["matchedid"]): x["status"] for x in u["user"]["items"]}
            Wm = [i for (y, i), s in last.items() if y == 0 and s not in (3, 5)]
            Wo = [i for (y, i), s in last.items() if y == 1 and s not in (3, 5)]
            Km = [i for (y, i), s in last.items() if y == 0 and s in (1, 2, 6)]
            hits["adapt"] += int((rr._reach(ada, Wo, 60) & ~rr._reach(dep, Wm, 60)).sum())
            hits["recap"] += int(rr._reach(rec, Wm, 60).sum())
            hits["sequel"] += int(rr._reach(dep, Km, 60).sum())
        hits["missing_dep"] += int(rr.dense(dep).any(1).sum())
    assert all(v > 0 for v in hits.values()), hits


def test_literal_prior_is_the_fp64_prior_in_float32():
    rng = np.random.default_rng(3)
    V, dim = (50, 70), 16
    sim = {f"embeddings.{m}": rng.standard_normal((dim, V[m])).astype(np.float32) for m in (0, 1)}
    sim.update({f"crossproject.{m}": rng.standard_normal((dim, dim)).astype(np.float32) for m in (0, 1)})
    st = dict(medium=1, users=[], items=[dict(medium=0, matchedid=4), dict(medium=1, matchedid=9), dict(medium=1, matchedid=9)])
    p32 = rr.prior_literal(1, sim, st, V)
    p64 = rr.prior_fp64(1, sim, st, V)
    assert np.allclose(p32, p64, rtol=1e-5, atol=1e-4)
    assert np.array_equal(rr.prior_fp64(1, sim, dict(medium=1, users=[], items=[]), V), np.zeros(V[1]))


# ---------------------------------------------------------------- host packing (the C entry point recorded, not called)
class _Recorder:
    """stands in for the library: rsys_retrieve_request reads its arguments back through the pointers it is given"""

    def __init__(self, D):
        self.D, self.calls = D, []

    def rsys_retrieve_request(self, h, medium, q, nq, group, ng, hoff, hmed, hid, hst, soff, smed, sid, k, ids, scores, counts):
        arr = lambda p, t, n: None if p is None else np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), (n,)).copy()
        H = arr(hoff, C.c_int64, nq + 1)
        S = arr(soff, C.c_int64, ng + 1)
        nh = 0 if H is None else int(H[-1])
        ns = 0 if S is None else int(S[-1])
        self.calls.append(dict(medium=medium, q=arr(q, C.c_float, nq * self.D).reshape(nq, self.D), group=arr(group, C.c_int32, nq),
                               ng=ng, hoff=H, hmed=arr(hmed, C.c_int32, nh), hid=arr(hid, C.c_int32, nh), hst=arr(hst, C.c_int32, nh),
                               soff=S, smed=arr(smed, C.c_int32, ns), sid=arr(sid, C.c_int32, ns), k=k))
        ids = np.ctypeslib.as_array(C.cast(ids, C.POINTER(C.c_int32)), (ng * k,))
        sc = np.ctypeslib.as_array(C.cast(scores, C.POINTER(C.c_float)), (ng * k,))
        cnt = np.ctypeslib.as_array(C.cast(counts, C.POINTER(C.c_int32)), (ng,))
        ids[:] = np.tile(np.arange(k, dtype=np.int32), ng)
        sc[:] = -np.arange(ng * k, dtype=np.float32)
        cnt[:] = np.arange(1, ng + 1, dtype=np.int32)
        return 0


def _fake_model(monkeypatch, V=(30, 40), D=8):
    from recommendersystem_amd import model as model_mod
    rec = _Recorder(D)
    monkeypatch.setattr(model_mod, "lib", lambda: rec)
    m = model_mod.RecommenderModel.__new__(model_mod.RecommenderModel)
    m._h = None
    m.config = {"vocab_sizes": {"0_matchedid": V[0], "1_matchedid": V[1]}, "embed_dim": D}
    return m, rec


def test_serve_retrieval_packs_render_states(monkeypatch):
    from recommendersystem_amd import serve
    model, rec = _fake_model(monkeypatch)
    rng = np.random.default_rng(0)
    emb = lambda: {"1.retrieval": rng.standard_normal(8).tolist(), "0.retrieval": rng.standard_normal(8).tolist()}
    it = lambda y, i, s: dict(medium=y, matchedid=i, status=s, rating=0)
    states = [
        dict(medium=1, items=[dict(medium=0, matchedid=3), dict(medium=1, matchedid=7)],
             users=[dict(embeds=emb(), user=dict(items=[it(1, 5, 7), it(0, 2, 3), it(1, 5, 6)])),
                    dict(embeds=emb(), user=dict(items=[]))]),
        dict(medium=0, items=[], users=[dict(embeds=emb(), user=dict(items=[it(0, 1, 2)]))]),
        dict(medium=1, items=[dict(medium=1, matchedid=0)], users=[dict(embeds=emb(), user=dict(items=[it(0, 29, 1), it(1, 39, 8)]))]),
    ]
    out = serve.retrieval(model, states, k=1024, coefs=[0.5])
    assert len(rec.calls) == 2
    c0, c1 = rec.calls                                    # medium 0 first, then medium 1 (states 0 and 2)
    assert c0["medium"] == 0 and c0["ng"] == 1 and c0["k"] == 30 and c0["group"].tolist() == [0]
    assert c0["hoff"].tolist() == [0, 1] and c0["hmed"].tolist() == [0] and c0["hid"].tolist() == [1] and c0["hst"].tolist() == [2]
    assert c0["soff"].tolist() == [0, 0]
    assert np.array_equal(c0["q"][0], np.float32(states[1]["users"][0]["embeds"]["0.retrieval"]))
    assert c1["medium"] == 1 and c1["ng"] == 2 and c1["k"] == 40 and c1["group"].tolist() == [0, 0, 1]
    assert c1["hoff"].tolist() == [0, 3, 3, 5]
    assert c1["hmed"].tolist() == [1, 0, 1, 0, 1] and c1["hid"].tolist() == [5, 2, 5, 29, 39]
    assert c1["hst"].tolist() == [7, 3, 6, 1, 8]          # in list order, undeduplicated
    assert c1["soff"].tolist() == [0, 2, 3] and c1["smed"].tolist() == [0, 1, 1] and c1["sid"].tolist() == [3, 7, 0]
    q = np.float32([states[0]["users"][0]["embeds"]["1.retrieval"], states[0]["users"][1]["embeds"]["1.retrieval"],
                    states[2]["users"][0]["embeds"]["1.retrieval"]])
    assert np.array_equal(c1["q"], q)
    # results go back to the states in their order: counts from the recorder are 1 (first group) and 2 (second)
    assert [o[0].size for o in out] == [1, 1, 2]
    assert out[1][0].tolist() == [0] and out[2][0].tolist() == [0, 1]
    np.testing.assert_allclose(out[0][1], np.float32(0 + 2 * np.log(0.5)), rtol=1e-6)      # two users: + 2 log(coef)
    np.testing.assert_allclose(out[2][1], np.float32([-40, -41]) + np.float32(np.log(0.5)), rtol=1e-6)


def test_retrieve_request_argument_shapes(monkeypatch):
    model, rec = _fake_model(monkeypatch)
    q = np.zeros((3, 8), np.float32)
    with pytest.raises(ValueError):
        model.retrieve_request(q, 0, 5, histories=[[]])                       # one list per query
    with pytest.raises(ValueError):
        model.retrieve_request(q, 0, 5, group=[0, 0, 1], selected=[[]])      # one list per group
    with pytest.raises(ValueError):
        model.retrieve_request(q, 0, 5, group=[0, 1])
    ids, sc, cnt = model.retrieve_request(q, 0, 5, group=[0, 0, 1], histories=None, selected=None)
    c = rec.calls[-1]
    assert c["hoff"] is None and c["soff"] is None and ids.shape == (2, 5) and cnt.tolist() == [1, 2]


class _TableRecorder:
    def __init__(self, V):
        self.config = {"vocab_sizes": {"0_matchedid": V[0], "1_matchedid": V[1]}}
        self.rel, self.sim, self.released = {}, {}, {}

    def set_retrieval_relations(self, medium, *mats):
        from recommendersystem_amd.model import csc_parts
        self.rel[medium] = [csc_parts(a) for a in mats]

    def set_item_similarity(self, medium, embeddings, crossproject=None):
        self.sim[medium] = (np.asarray(embeddings), None if crossproject is None else np.asarray(crossproject))

    def set_released(self, medium, x):
        self.released[medium] = x


class _ScipyLike:
    def __init__(self, t):
        self.indptr, self.indices, self.data, self.shape = t


def test_load_retrieval_tables_accepts_julia_and_tuple_inputs():
    from recommendersystem_amd import serve
    rng = np.random.default_rng(5)
    V, dim = (12, 9), 8
    rel = rr.random_relations(rng, V, density=0.2)
    julia = lambda t: dict(colptr=t[0] + 1, rowval=t[1].astype(np.int64) + 1, nzval=t[2], m=t[3][0], n=t[3][1])   # 1-based
    relations = {}
    for m in (0, 1):
        relations[f"{m}.dependencies"] = julia(rel[f"{m}.dependencies"])           # Julia SparseMatrixCSC fields
        relations[f"{m}.recaps"] = rel[f"{m}.recaps"]                              # 0-based tuple
        relations[f"{m}.adaptations"] = _ScipyLike(rel[f"{m}.adaptations"])       # scipy-like object
    E = {m: rng.standard_normal((dim, V[m])).astype(np.float32) for m in (0, 1)}
    Cp = rng.standard_normal((dim, dim)).astype(np.float32)
    sim = {"embeddings.0": E[0], "embeddings.1": E[1].T, "crossproject.0": Cp}       # Julia's dim x V, and its transpose
    model = _TableRecorder(V)
    mask = rng.random(V[1]) < 0.5
    serve.load_retrieval_tables(model, relations, sim, released={1: mask})
    for m in (0, 1):
        got = model.rel[m]
        for kind, name in enumerate(serve.RELATION_KINDS):
            want = rel[f"{m}.{name}"]
            for a, b in zip(got[kind][:3], want[:3]):
                assert np.array_equal(a, b), (m, name)
            assert got[kind][3] == want[3]
        assert np.array_equal(model.sim[m][0], E[m].T)                            # (V_m, dim) rows
    assert np.array_equal(model.sim[0][1], Cp) and model.sim[1][1] is None
    assert 0 not in model.released and model.released[1] is mask


def test_csc_parts_checks_shapes():
    from recommendersystem_amd.model import csc_parts
    ip, ix, d, sh = csc_parts((np.array([0, 1, 1]), np.array([2, 7]), np.array([1.0, 9.0]), (3, 2)))
    assert ip.dtype == np.int64 and ix.dtype == np.int32 and d.dtype == np.float32 and sh == (3, 2)
    assert ix.tolist() == [2] and d.tolist() == [1.0]                            # trimmed to indptr[-1]
    with pytest.raises(ValueError):
        csc_parts((np.array([0, 1]), np.array([0]), np.array([1.0]), (3, 2)))      # indptr needs n_cols + 1 entries
    with pytest.raises(ValueError):
        csc_parts((np.array([0, 1, 3]), np.array([0]), np.array([1.0]), (3, 2)))   # fewer entries than indptr[-1]
