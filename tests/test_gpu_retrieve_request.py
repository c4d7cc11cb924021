"""GPU: whole retrieval requests on the device (rsys_retrieve_request: Inference/render.jl:240-331).  The masks are checked as exact
sets against the numpy restatement (tests/_render_retrieval_np.py), and bit for bit against rsys_retrieve_topk given the
restatement's masked ids as exclusions; the item-similarity prior against an fp64 restatement; plus the released filter,
reproducibility, isolation from training, and argument errors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_retrieval_np as rr  # noqa: E402

pytestmark = pytest.mark.gpu

TASK_W = [0.05, 0.2, 0.3, 0.25]
DIM = 64


def _model(dtype, vocab=None, seed=9, deterministic=False):
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config("hd64", mask_rate=0.2, mask_topk=16)
    if vocab:
        cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"] = vocab
    if deterministic:
        cfg["deterministic"] = True
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=4)
    if vocab:
        model.init_weights(seed)
        model.random_pretrained_embeddings(seed + 1)
    else:
        model.load_state_dict(synth.make_params(cfg, seed, "test"))
    V = (cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"])
    return cfg, model, V


def _similarity(rng, V, dim=DIM):
    sim = {f"embeddings.{m}": (0.3 * rng.standard_normal((dim, V[m]))).astype(np.float32) for m in (0, 1)}
    sim.update({f"crossproject.{m}": (rng.standard_normal((dim, dim)) / np.sqrt(dim)).astype(np.float32) for m in (0, 1)})
    return sim


def _load(model, rel, sim=None, released=None):
    from recommendersystem_amd import serve
    serve.load_retrieval_tables(model, rel, sim or {}, released)


def _args(states, m, D):
    """queries, group, histories, selected of a list of states (one group each); queries are random unit-scale vectors"""
    from recommendersystem_amd import serve
    rng = np.random.default_rng(len(states))
    for st in states:
        for u in st["users"]:
            u.setdefault("embeds", {f"{m}.retrieval": rng.standard_normal(D).astype(np.float32)})
    return serve.request_arrays(states, m)


def _bf16(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16
    return b.astype(np.uint32).view(np.float32)


def _logp(model, cfg, dtype, q, m):
    n0 = cfg["vocab_sizes"]["0_matchedid"]
    F = model.item_embeddings()
    F = F[:n0] if m == 0 else F[n0:]
    if dtype == "bf16":
        F, q = _bf16(F), _bf16(q)
    z = F.astype(np.float64) @ q.astype(np.float64).T
    zmax = z.max(0)
    return (z - (zmax + np.log(np.exp(z - zmax).sum(0)))).T               # (n, V_m)


def _check_e2e(ids, scores, counts, ref, adm, k, tol_rel):
    for g in range(ref.shape[0]):
        n = int(counts[g])
        assert n == min(k, int(adm[g].sum())), (g, n)
        got = ids[g, :n]
        assert (ids[g, n:] == -1).all() and np.isneginf(scores[g, n:]).all()
        assert len(set(got.tolist())) == n and adm[g, got].all()
        tol = tol_rel * np.maximum(1.0, np.abs(ref[g, got]))
        assert (np.abs(scores[g, :n] - ref[g, got]) <= tol).all(), np.abs(scores[g, :n] - ref[g, got]).max()
        assert (np.diff(scores[g, :n]) <= 0).all()
        if n:
            rest = adm[g].copy(); rest[got] = False
            lo = scores[g, n - 1]
            assert (ref[g, rest] <= lo + 2 * tol_rel * max(1.0, abs(lo))).all()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_masks_are_the_restatements_set(dtype):
    cfg, model, V = _model(dtype)
    rng = np.random.default_rng(11)
    rel = rr.random_relations(rng, V, density=0.03)
    sim = _similarity(rng, V)
    _load(model, rel, sim)
    for m in (0, 1):
        states = [rr.random_state(rng, V, m, n_users=int(rng.integers(1, 4)), n_items=60, n_selected=int(rng.integers(0, 4)))
                  for _ in range(5)]
        q, group, hist, sel = _args(states, m, cfg["embed_dim"])
        k = V[m]
        ids, sc, cnt = model.retrieve_request(q, m, k, group=group, histories=hist, selected=sel)
        for g, st in enumerate(states):
            want = np.flatnonzero(~rr.set_mask(m, rel, st, V))
            _, adm = rr.literal(m, rel, st, V)
            assert np.array_equal(want, np.flatnonzero(adm))
            assert cnt[g] == want.size
            assert np.array_equal(np.sort(ids[g, :cnt[g]]), want)
            assert (ids[g, cnt[g]:] == -1).all()
    model.close()


def test_masks_through_the_existing_pipeline_bit_for_bit():
    cfg, model, V = _model("fp32", vocab=(60000, 40000))
    rng = np.random.default_rng(12)
    rel = {}
    for m in (0, 1):        # about three entries per column, some explicit zeros, a quarter of the rows empty in dependencies
        rel[f"{m}.dependencies"] = rr.random_csc(rng, V[m], V[m], 3.0 / V[m], empty_rows=rng.choice(V[m], V[m] // 4, replace=False))
        rel[f"{m}.recaps"] = rr.random_csc(rng, V[m], V[m], 1.0 / V[m])
        rel[f"{m}.adaptations"] = rr.random_csc(rng, V[m], V[1 - m], 2.0 / V[1 - m])
    _load(model, rel)
    for m in (0, 1):
        states = [rr.random_state(rng, V, m, n_users=int(rng.integers(1, 4)), n_items=400, n_selected=0) for _ in range(16)]
        q, group, hist, sel = _args(states, m, cfg["embed_dim"])
        k = 1024
        a = model.retrieve_request(q, m, k, group=group, histories=hist, selected=sel)
        excl = [np.flatnonzero(rr.set_mask(m, rel, st, V)) for st in states]
        b = model.retrieve_topk(q, m, k, group=group, exclude=excl)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_prior_of_selected_items(dtype):
    cfg, model, V = _model(dtype, vocab=(3000, 2000))
    tol_rel = 2e-5 if dtype == "fp32" else 2e-3
    rng = np.random.default_rng(13)
    rel = rr.random_relations(rng, V, density=0.0005)
    sim = _similarity(rng, V)
    released = {m: rng.random(V[m]) < 0.9 for m in (0, 1)}
    _load(model, rel, sim, released)
    for m in (0, 1):
        states = []
        for j in range(9):
            st = rr.random_state(rng, V, m, n_users=1 + j % 2, n_items=50, n_selected=j % 5)
            if j == 8:   # duplicates, both media
                st["items"] = [dict(medium=1 - m, matchedid=5), dict(medium=m, matchedid=7), dict(medium=1 - m, matchedid=5)]
            states.append(st)
        q, group, hist, sel = _args(states, m, cfg["embed_dim"])
        lp = _logp(model, cfg, dtype, q, m)
        k = 1024
        ids, sc, cnt = model.retrieve_request(q, m, k, group=group, histories=hist, selected=sel)
        ref = np.stack([rr.prior_fp64(m, sim, st, V) for st in states])
        for i, g in enumerate(group):
            ref[g] += lp[i]
        adm = np.stack([~rr.set_mask(m, rel, st, V, released=released[m]) for st in states])
        _check_e2e(ids, sc, cnt, ref, adm, k, tol_rel)
    model.close()


def test_released_filter_and_item_zero():
    cfg, model, V = _model("fp32")
    rng = np.random.default_rng(14)
    empty = {f"{m}.{kind}": (np.zeros(V[m if kind != "adaptations" else 1 - m] + 1, np.int64), np.zeros(0, np.int32),
                             np.zeros(0, np.float32), (V[m], V[m] if kind != "adaptations" else V[1 - m]))
             for m in (0, 1) for kind in ("dependencies", "recaps", "adaptations")}
    _load(model, empty)
    q = rng.standard_normal((2, cfg["embed_dim"])).astype(np.float32)
    for m in (0, 1):
        mask = rng.random(V[m]) < 0.6
        model.set_released(m, mask)
        ids, sc, cnt = model.retrieve_request(q, m, V[m])
        for g in range(2):
            got = ids[g, :cnt[g]]
            assert 0 not in got and mask[got].all()
            assert cnt[g] == int(mask[1:].sum())
        model.set_released(m, np.flatnonzero(mask))                       # ids instead of a mask: the same set
        ids2, sc2, cnt2 = model.retrieve_request(q, m, V[m])
        assert ids2.tobytes() == ids.tobytes() and sc2.tobytes() == sc.tobytes()
        model.set_released(m, None)
        ids, sc, cnt = model.retrieve_request(q, m, V[m])
        assert (cnt == V[m] - 1).all()
        assert np.array_equal(np.sort(ids[0, :cnt[0]]), np.arange(1, V[m]))        # the unreleased items are back, item 0 is not
    model.close()


def test_reproducible_and_follows_the_table():
    cfg, model, V = _model("bf16")
    rng = np.random.default_rng(15)
    rel = rr.random_relations(rng, V, density=0.03)
    _load(model, rel, _similarity(rng, V))
    states = [rr.random_state(rng, V, 1, 2, 40, 3) for _ in range(3)]
    q, group, hist, sel = _args(states, 1, cfg["embed_dim"])
    run = lambda: model.retrieve_request(q, 1, 150, group=group, histories=hist, selected=sel)
    a, b = run(), run()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    name = "item_embedding.projection_layer.bias"
    bias = model.get_parameter(name)
    model.set_parameter(name, bias + rng.standard_normal(bias.shape).astype(np.float32))
    c = run()
    assert c[1].tobytes() != a[1].tobytes()            # the fused table was rebuilt
    model.set_parameter(name, bias)
    d = run()
    for x, y in zip(a, d):
        assert x.tobytes() == y.tobytes()
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_request_between_training_steps_changes_nothing(dtype):
    """Deterministic mode: step -> load tables + retrieve_request -> step gives the step -> step results bit for bit."""
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config("hd64", mask_rate=0.2, deterministic=True)
    V = (cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"])
    P = synth.make_params(cfg, 3, "test")
    rows = 4
    batches = [synth.make_batch(cfg, rows, 40 + i) for i in range(2)]
    masks = [synth.make_masks(cfg, rows, 50 + i) for i in range(2)]
    names = synth.trainable_names(cfg)
    rng = np.random.default_rng(16)
    rel = rr.random_relations(rng, V, density=0.03)
    sim = _similarity(rng, V)
    states = [rr.random_state(rng, V, 0, 2, 30, 2) for _ in range(2)]
    q, group, hist, sel = _args(states, 0, cfg["embed_dim"])

    def run(retrieve):
        model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
        model.load_state_dict(P)
        opt = ra.create_optimizer(model, dict(cfg, learning_rate=1e-2))
        model.set_loss_weights(TASK_W, 1)
        out = []
        for i, (d, mk) in enumerate(zip(batches, masks)):
            if i == 1 and retrieve:
                _load(model, rel, sim, {0: rng.random(V[0]) < 0.8})
                model.retrieve_request(q, 0, 50, group=group, histories=hist, selected=sel)
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
    from recommendersystem_amd import _lib
    cfg, model, V = _model("fp32")
    D = cfg["embed_dim"]
    rng = np.random.default_rng(17)
    q = rng.standard_normal((2, D)).astype(np.float32)
    with pytest.raises(ra.RsysError):                                      # no relation tables yet
        model.retrieve_request(q, 0, 5)
    rel = rr.random_relations(rng, V, density=0.05)
    _load(model, rel)
    dep = rel["0.dependencies"]
    L = ra.lib()

    def setrel(medium, kind, n_rows, n_cols, ip, ix, d):
        ip = np.ascontiguousarray(ip, np.int64); ix = np.ascontiguousarray(ix, np.int32); d = np.ascontiguousarray(d, np.float32)
        _lib.check(L.rsys_retrieve_relations_set(model._h, medium, kind, n_rows, n_cols, ip.ctypes.data, ix.ctypes.data, d.ctypes.data))

    ip, ix, d, (nr, nc) = dep
    nz = int(ip[-1])
    bad_vals = d.copy(); bad_vals[nz // 2] = -1.0
    nan_vals = d.copy(); nan_vals[nz // 3] = np.nan
    bad_ip = ip.copy(); bad_ip[5] = bad_ip[6] + 1
    bad_ix = ix.copy(); bad_ix[0] = nr
    bad = [
        (0, 0, nr + 1, nc, ip, ix, d),                        # wrong shape
        (0, 2, nr, nc, ip, ix, d),                            # adaptations are V_0 x V_1
        (0, 0, nr, nc, ip, ix, bad_vals),                     # negative value
        (0, 0, nr, nc, ip, ix, nan_vals),                     # NaN
        (0, 0, nr, nc, bad_ip, ix, d),                        # colptr not monotone
        (0, 0, nr, nc, ip, bad_ix, d),                        # row out of range
        (0, 3, nr, nc, ip, ix, d),                            # kind outside 0..2
        (2, 0, nr, nc, ip, ix, d),                            # medium
    ]
    for args in bad:
        with pytest.raises(ra.RsysError):
            setrel(*args)
    model.retrieve_request(q, 0, 5)                           # the loaded tables still stand
    # request arguments
    sim = _similarity(rng, V)
    model.set_item_similarity(1, sim["embeddings.1"].T)       # medium 1 without its crossproject
    bad_req = [
        dict(histories=[[(0, V[0], 7)], []]),                 # id out of range for its medium
        dict(histories=[[(2, 1, 7)], []]),                    # medium
        dict(selected=[[(0, 3)], []]),                        # similarity of medium 0 not loaded
        dict(selected=[[(1, V[1])], []]),                     # out of range
    ]
    for kw in bad_req:
        with pytest.raises(ra.RsysError):
            model.retrieve_request(q, 0, 5, **kw)
    model.set_item_similarity(0, sim["embeddings.0"].T, sim["crossproject.0"].T)
    with pytest.raises(ra.RsysError):                         # crossproject of medium 1 missing for a cross-medium item
        model.retrieve_request(q, 0, 5, selected=[[(1, 3)], []])
    model.retrieve_request(q, 0, 5, selected=[[(0, 3)], []])
    model.set_item_similarity(1, sim["embeddings.1"].T, sim["crossproject.1"].T)
    model.retrieve_request(q, 0, 5, selected=[[(1, 3)], []])
    # malformed offsets through the C entry point
    ids = np.empty((2, 5), np.int32); sc = np.empty((2, 5), np.float32); cnt = np.empty(2, np.int32)
    off = np.array([0, 2, 1], np.int64); z = np.zeros(2, np.int32)
    with pytest.raises(ra.RsysError):
        _lib.check(L.rsys_retrieve_request(model._h, 0, q.ctypes.data, 2, None, 2, off.ctypes.data, z.ctypes.data, z.ctypes.data,
                                           z.ctypes.data, None, None, None, 5, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data))
    with pytest.raises(ra.RsysError):
        _lib.check(L.rsys_retrieve_request(model._h, 0, q.ctypes.data, 2, None, 2, None, None, None, None, off.ctypes.data,
                                           z.ctypes.data, z.ctypes.data, 5, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data))
    with pytest.raises(ra.RsysError):                         # missing table of the request medium
        model.set_retrieval_relations(1, None, rel["1.recaps"], rel["1.adaptations"])
        model.retrieve_request(q, 1, 5)
    model.retrieve_request(q, 0, 5)                           # still usable
    model.close()
