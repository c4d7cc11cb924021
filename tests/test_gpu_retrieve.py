"""GPU: retrieval top-k on the device (rsys_retrieve_topk / rsys_op_topk; Finetune/embed.jl:86-90 + the scoring, masking and sort of
Inference/render.jl:240-333).  The selection is checked bit for bit against a stable numpy sort; the whole call against an fp64
restatement on the same operands (the model's fused item table and its inference_select queries, rounded to bf16 in bf16 mode)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _retrieve_np import _expect_topk, _rows  # noqa: E402

pytestmark = pytest.mark.gpu

TASK_W = [0.05, 0.2, 0.3, 0.25]


# ---------------------------------------------------------------- rsys_op_topk against np.lexsort
def _op_topk(scores, k, ld=None):
    from recommendersystem_amd._lib import check, lib
    rows, V = scores.shape
    ld = V if ld is None else ld
    host = np.full((rows, ld), np.nan, np.float32)
    host[:, :V] = scores
    L = lib()
    ptrs = []
    for nbytes in (host.nbytes, rows * k * 4, rows * k * 4, rows * 4):
        p = C.c_void_p()
        check(L.rsys_dev_alloc(C.byref(p), nbytes))
        ptrs.append(p)
    try:
        check(L.rsys_dev_h2d(ptrs[0], host.ctypes.data, host.nbytes))
        check(L.rsys_op_topk(ptrs[0], ld, rows, V, k, ptrs[1], ptrs[2], ptrs[3]))
        ids = np.empty((rows, k), np.int32); vals = np.empty((rows, k), np.float32); counts = np.empty(rows, np.int32)
        check(L.rsys_dev_d2h(ids.ctypes.data, ptrs[1], ids.nbytes))
        check(L.rsys_dev_d2h(vals.ctypes.data, ptrs[2], vals.nbytes))
        check(L.rsys_dev_d2h(counts.ctypes.data, ptrs[3], counts.nbytes))
    finally:
        for p in ptrs:
            L.rsys_dev_free(p)
    return ids, vals, counts


def _check_op(scores, k, ld=None):
    ids, vals, counts = _op_topk(scores, k, ld)
    for r in range(scores.shape[0]):
        e_ids, e_vals = _expect_topk(scores[r], k)
        n = e_ids.size
        assert counts[r] == n, (r, counts[r], n)
        assert np.array_equal(ids[r, :n], e_ids), r
        assert np.array_equal(vals[r, :n].view(np.uint32), e_vals.view(np.uint32)), r
        assert (ids[r, n:] == -1).all() and np.isneginf(vals[r, n:]).all(), r


@pytest.mark.parametrize("kind", ["random", "equal", "ulp", "zeros", "special"])
@pytest.mark.parametrize("V,rows", [(119999, 1), (119999, 64), (37, 1), (37, 64)])
def test_op_topk_is_a_stable_sort(kind, V, rows):
    rng = np.random.default_rng(V + rows)
    x = _rows(kind, rows, V, rng)
    ks = {1, V, min(V, 8192), min(V, 1024)}
    if kind == "special":
        ks.add(min(V, 8192))   # above the admissible count of the -inf-heavy rows
    for k in sorted(ks):
        if k > 8192:
            continue
        _check_op(x, k)


def test_op_topk_row_stride_and_more_than_admissible():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 1000)).astype(np.float32)
    x[:, 10:] = -np.inf                        # 10 admissible, k = 500
    _check_op(x, 500, ld=1024)
    ids, vals, counts = _op_topk(x, 500, ld=1024)
    assert (counts == 10).all()


def test_op_topk_argument_errors():
    import recommendersystem_amd as ra
    x = np.zeros((1, 16), np.float32)
    for k in (0, 17):
        with pytest.raises(ra.RsysError):
            _op_topk(x, k)


# ---------------------------------------------------------------- end to end
def _model(name, dtype, vocab=None, seed=9, deterministic=False):
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config(name, mask_rate=0.2, mask_topk=16)
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
    return cfg, model


def _queries(cfg, model, n, seed):
    """n retrieval embeddings from the inference forward (inference_select at random tokens of a synthetic batch)."""
    from oracle import synth
    rows = 4
    S = cfg["max_sequence_length"]
    d = synth.make_batch(cfg, rows, seed)
    d["rope_input_pos"] = np.tile(np.arange(S, dtype=np.int32), rows)
    idx = np.random.default_rng(seed).choice(rows * 2 * S, size=n, replace=False).astype(np.int32)
    return model.inference_select(d, "retrieval", idx)


def _bf16(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16                 # round to nearest even
    return b.astype(np.uint32).view(np.float32)


def _reference(model, cfg, dtype, q, medium, group, ng, prior, exclude):
    n0 = cfg["vocab_sizes"]["0_matchedid"]
    F = model.item_embeddings()
    F = F[:n0] if medium == 0 else F[n0:]
    if dtype == "bf16":
        F, q = _bf16(F), _bf16(q)
    z = F.astype(np.float64) @ q.astype(np.float64).T                # (V_m, n)
    zmax = z.max(0)
    lse = zmax + np.log(np.exp(z - zmax).sum(0))
    lp = (z - lse).T                                                  # (n, V_m)
    score = np.zeros((ng, F.shape[0])) if prior is None else prior.astype(np.float64).copy()
    for i, g in enumerate(group):
        score[g] += lp[i]
    adm = np.isfinite(score) | (score == np.inf)
    if exclude is not None:
        for g in range(ng):
            adm[g, np.asarray(exclude[g], np.int64)] = False
    return score, adm, lp


def _check_e2e(ids, scores, counts, ref, adm, k, tol_rel):
    for g in range(ref.shape[0]):
        n = int(counts[g])
        assert n == min(k, int(adm[g].sum())), (g, n)
        got = ids[g, :n]
        assert (ids[g, n:] == -1).all() and np.isneginf(scores[g, n:]).all()
        assert len(set(got.tolist())) == n and adm[g, got].all()           # admissible, no duplicates (exclusions honoured)
        tol = tol_rel * np.maximum(1.0, np.abs(ref[g, got]))
        assert (np.abs(scores[g, :n] - ref[g, got]) <= tol).all(), np.abs(scores[g, :n] - ref[g, got]).max()
        assert (np.diff(scores[g, :n]) <= 0).all()                         # non-increasing
        if n:
            rest = adm[g].copy(); rest[got] = False
            lo = scores[g, n - 1]
            assert (ref[g, rest] <= lo + 2 * tol_rel * max(1.0, abs(lo))).all()   # a valid top-k


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name,vocab", [("hd64", None), ("hd64", (60000, 40000))])
def test_retrieve_topk_end_to_end(dtype, name, vocab):
    cfg, model = _model(name, dtype, vocab)
    tol_rel = 2e-5 if dtype == "fp32" else 2e-3
    q = _queries(cfg, model, 7, 21)
    rng = np.random.default_rng(1)
    for medium in (0, 1):
        Vm = cfg["vocab_sizes"][f"{medium}_matchedid"]
        k = min(Vm, 1024 if vocab else 64)
        # one group per query
        ids, sc, cnt = model.retrieve_topk(q, medium, k)
        ref, adm, lp = _reference(model, cfg, dtype, q, medium, range(7), 7, None, None)
        _check_e2e(ids, sc, cnt, ref, adm, k, tol_rel)
        # groups: {0, 3} {1} {2, 4, 5, 6}; a prior with -inf entries; ragged exclusions with duplicates and item 0
        group = np.array([0, 1, 2, 0, 2, 2, 2], np.int32)
        prior = rng.standard_normal((3, Vm)).astype(np.float32)
        prior[rng.random((3, Vm)) < 0.2] = -np.inf
        exclude = [np.array([0, 5, 5, Vm - 1]), np.array([], np.int64), rng.integers(0, Vm, 40)]
        ids, sc, cnt = model.retrieve_topk(q, medium, k, group=group, prior=prior, exclude=exclude)
        ref, adm, lp = _reference(model, cfg, dtype, q, medium, group, 3, prior, exclude)
        _check_e2e(ids, sc, cnt, ref, adm, k, tol_rel)
        # a two-user group is the sum of its members' log-probabilities
        ids, sc, cnt = model.retrieve_topk(q[[0, 3]], medium, k, group=[0, 0])
        two = lp[0] + lp[3]
        assert np.abs(sc[0] - two[ids[0]]).max() <= tol_rel * 2 * max(1.0, np.abs(two).max())
        # k = V_m: every item, counts and padding with an exclusion list
        kk = min(Vm, 8192)
        ids, sc, cnt = model.retrieve_topk(q[:1], medium, kk, exclude=[np.arange(0, Vm, 2)])
        assert cnt[0] == min(kk, Vm - (Vm + 1) // 2) and (ids[0, :cnt[0]] % 2 == 1).all()
        assert (ids[0, cnt[0]:] == -1).all()
    model.close()


def test_retrieve_topk_is_reproducible_and_follows_the_table():
    cfg, model = _model("hd64", "bf16")
    q = _queries(cfg, model, 5, 4)
    a = model.retrieve_topk(q, 1, 150, group=[0, 1, 0, 1, 1])
    b = model.retrieve_topk(q, 1, 150, group=[0, 1, 0, 1, 1])
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    name = "item_embedding.projection_layer.bias"
    bias = model.get_parameter(name)
    rng = np.random.default_rng(2)
    model.set_parameter(name, bias + rng.standard_normal(bias.shape).astype(np.float32))
    c = model.retrieve_topk(q, 1, 150, group=[0, 1, 0, 1, 1])
    assert c[1].tobytes() != a[1].tobytes()            # the fused table was rebuilt
    model.set_parameter(name, bias)
    d = model.retrieve_topk(q, 1, 150, group=[0, 1, 0, 1, 1])
    for x, y in zip(a, d):
        assert x.tobytes() == y.tobytes()
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_retrieve_between_training_steps_changes_nothing(dtype):
    """Deterministic mode: step -> retrieve -> step gives the losses, gradients and parameters of step -> step, bit for bit."""
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config("hd64", mask_rate=0.2, deterministic=True)
    P = synth.make_params(cfg, 3, "test")
    rows = 4
    batches = [synth.make_batch(cfg, rows, 40 + i) for i in range(2)]
    masks = [synth.make_masks(cfg, rows, 50 + i) for i in range(2)]
    q = np.random.default_rng(0).standard_normal((3, cfg["embed_dim"])).astype(np.float32)
    names = synth.trainable_names(cfg)

    def run(retrieve):
        model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
        model.load_state_dict(P)
        opt = ra.create_optimizer(model, dict(cfg, learning_rate=1e-2))
        model.set_loss_weights(TASK_W, 1)
        out = []
        for i, (d, mk) in enumerate(zip(batches, masks)):
            if i == 1 and retrieve:
                model.retrieve_topk(q, 0, 50)
                model.retrieve_topk(q, 1, 50, group=[0, 0, 0])
            out.append(np.array(model(d, False, masks=mk), np.float32))
            out += [model.grad(n).copy() for n in names]
            opt.step(clip_max_norm=1.0)
        out += [model.get_parameter(n).copy() for n in names]
        model.close()
        return out

    a, b = run(False), run(True)
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_serve_retrieve_matches_compute_retrieval(tmp_path):
    """serve.retrieve (device) against serve.compute_retrieval + argsort on the registry (host, fp64) for an fp32 model with a
    retrieval coefficient: same scores up to tolerance, the same ranking up to near-ties."""
    import recommendersystem_amd as ra
    from recommendersystem_amd import h5, serve
    if not os.path.exists(h5.LIB_PATH):
        pytest.skip("librsys_h5.so not built (no libhdf5 on this host)")
    cfg, model = _model("hd64", "fp32")
    q = _queries(cfg, model, 3, 8)
    path = str(tmp_path / "model.registry.h5")
    serve.register_transformer(model, path)
    reg = h5.read_h5(path)
    coef = 0.37
    reg["0.retrieval.coefs"] = np.array([coef], np.float32)
    embeds = [{"0.retrieval": v.tolist()} for v in q]
    k = 100
    got = serve.retrieve(model, embeds, 0, k, groups=[0, 0, 1], exclude=[[0, 1, 2], [0]], coefs=reg["0.retrieval.coefs"])
    n0 = cfg["vocab_sizes"]["0_matchedid"]
    for g, members, excl in ((0, [0, 1], [0, 1, 2]), (1, [2], [0])):
        probs = [serve.compute_retrieval(reg, 0, embeds[i]).astype(np.float64) for i in members]
        assert all(pr.shape == (n0,) for pr in probs)
        p = np.sum([np.log(pr) for pr in probs], axis=0)
        adm = np.ones(n0, bool); adm[excl] = False
        ids, sc = got[g]
        assert ids.size == k
        _check_e2e(ids[None], sc[None], np.array([k]), p[None], adm[None], k, 2e-5)
        order = np.argsort(-np.where(adm, p, -np.inf), kind="stable")[:k]
        tol = 4e-5 * max(1.0, abs(p[order[-1]]))
        same = ids == order
        assert (same | (np.abs(p[ids] - p[order]) <= tol)).all()    # same ranking up to near-ties
    model.close()
    ra.synchronize()


def test_retrieve_topk_argument_errors():
    import recommendersystem_amd as ra
    from oracle import synth
    cfg, model = _model("hd64", "fp32")
    D = cfg["embed_dim"]
    q = np.zeros((2, D), np.float32)
    bad = [
        dict(queries=q, medium=2, k=5),
        dict(queries=q, medium=0, k=0),
        dict(queries=q, medium=0, k=121),                                  # > V_0 = 120
        dict(queries=q, medium=0, k=5, group=[0, 2]),                      # group 1 has no query
        dict(queries=np.zeros((4097, D), np.float32), medium=0, k=5),
        dict(queries=q, medium=0, k=5, exclude=[[120], []]),              # out of range
        dict(queries=q, medium=1, k=5, exclude=[[-1], []]),
    ]
    for kw in bad:
        with pytest.raises(ra.RsysError):
            model.retrieve_topk(**kw)
    model.retrieve_topk(q, 0, 5)                                           # still usable
    model.close()
    cfg = synth.make_config("hd64", mask_rate=0.2, mask_topk=16)
    cfg["table_shard"] = (0, 1)
    sh = ra.RecommenderModel(cfg, dtype="fp32", max_rows=2)
    with pytest.raises(ra.RsysError):
        sh.retrieve_topk(q, 0, 5)
    sh.close()


# ---------------------------------------------------------------- results do not depend on what the workspace held before
# A small call, a call sized to replace every buffer of the call family's workspace (257 queries: one row past the 256-query chunk),
# then the small call again: the second small call returns what the first did, bit for bit.  The three callers of the shared scoring
# prologue: retrieve_topk, retrieve_target_rank, rank_request.
def _same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_retrieve_topk_small_large_small(dtype):
    cfg, model = _model("hd64", dtype)
    tol_rel = 2e-5 if dtype == "fp32" else 2e-3
    rng = np.random.default_rng(31)
    D = cfg["embed_dim"]
    qa = rng.standard_normal((3, D)).astype(np.float32)
    qb = rng.standard_normal((257, D)).astype(np.float32)
    for medium in (0, 1):
        Vm = cfg["vocab_sizes"][f"{medium}_matchedid"]
        small = dict(queries=qa, medium=medium, k=8, group=[0, 1, 0], exclude=[np.array([0, 5, Vm - 1]), np.array([3])])
        a1 = model.retrieve_topk(**small)
        group = (np.arange(257) % 5).astype(np.int32)
        exclude = [rng.integers(0, Vm, 10) for _ in range(5)]
        k = min(Vm, 8192)
        ids, sc, cnt = model.retrieve_topk(qb, medium, k, group=group, exclude=exclude)
        a2 = model.retrieve_topk(**small)
        _same_bits(a1, a2)
        ref, adm, _ = _reference(model, cfg, dtype, qb, medium, group, 5, None, exclude)
        _check_e2e(ids, sc, cnt, ref, adm, k, tol_rel)
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_retrieve_target_rank_small_large_small(dtype):
    cfg, model = _model("hd64", dtype)
    tol_rel = 2e-5 if dtype == "fp32" else 2e-3
    rng = np.random.default_rng(32)
    D = cfg["embed_dim"]
    medium = 1
    Vm = cfg["vocab_sizes"]["1_matchedid"]
    qa = rng.standard_normal((3, D)).astype(np.float32)
    qb = rng.standard_normal((257, D)).astype(np.float32)
    small = dict(queries=qa, medium=medium, targets=[4, 0, Vm - 1], exclude=[np.array([1, 2]), np.array([], np.int64), np.array([Vm - 1])])
    a1 = model.retrieve_target_rank(**small)
    targets = rng.integers(0, Vm, 257).astype(np.int32)
    exclude = [np.setdiff1d(rng.integers(0, Vm, 6), [targets[i]]) for i in range(257)]
    rank, logp = model.retrieve_target_rank(qb, medium, targets, exclude=exclude)
    a2 = model.retrieve_target_rank(**small)
    _same_bits(a1, a2)
    assert a1[0][2] == 0                                                    # its target is excluded
    _, _, lp = _reference(model, cfg, dtype, qb, medium, range(257), 257, None, None)
    for i in range(257):
        t = lp[i, targets[i]]
        tol = tol_rel * max(1.0, abs(t))
        assert abs(logp[i] - t) <= tol, (i, logp[i], t)
        others = np.ones(Vm, bool)
        others[exclude[i]] = False
        others[targets[i]] = False
        lo = 1 + int((lp[i, others] > t + 2 * tol).sum())
        hi = 1 + int((lp[i, others] >= t - 2 * tol).sum())
        assert lo <= rank[i] <= hi, (i, rank[i], lo, hi)
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_rank_request_small_large_small(dtype):
    cfg, model = _model("hd64", dtype)
    rng = np.random.default_rng(33)
    D = cfg["embed_dim"]
    medium = 1
    Vm = cfg["vocab_sizes"]["1_matchedid"]
    model.set_item_similarity(medium, (0.3 * rng.standard_normal((Vm, 64))).astype(np.float32))
    cols = [np.unique(rng.integers(0, Vm, 4)) for _ in range(Vm)]
    indptr = np.concatenate([[0], np.cumsum([c.size for c in cols])])
    rows = np.concatenate(cols)
    model.set_related(medium, (indptr, rows, np.ones(rows.size, np.float32), (Vm, Vm)))

    def request(sizes, group):
        r = np.random.default_rng(34 + len(sizes))
        cand = [r.choice(Vm, n, replace=False).astype(np.int32) for n in sizes]
        q = r.standard_normal((len(group), D)).astype(np.float32)
        rm = [r.uniform(0, 10, sizes[g]).astype(np.float32) for g in group]
        hist = [[(medium, int(i), 2) for i in r.integers(0, Vm, 5)] for _ in group]
        pen = [(0.9, 0.3, 1.5, 0.5)] * len(sizes)
        ids, sc = model.rank_request(q, medium, cand, group=group, r_masked=rm, partialk=[n for n in sizes], penalties=pen, histories=hist)
        for g, n in enumerate(sizes):
            assert ids[g].size == n and set(ids[g].tolist()) <= set(cand[g].tolist())
        return ids + sc

    a1 = request([4], [0])
    request([64, 33, min(64, Vm)], [0, 1, 2, 0, 2])
    a2 = request([4], [0])
    _same_bits(a1, a2)
    model.close()
