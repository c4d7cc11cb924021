"""GPU: finetune evaluation on the device (rsys_retrieve_target_rank / rsys_op_target_rank; Finetune/regress.jl:193-331).  The count
alone bit for bit against numpy on adversarial rows; the whole call against rsys_retrieve_topk's lists (position and score of the target)
and against an fp64 restatement on the same operands; chunking, reproducibility, isolation from training, argument errors; and
regress.save_weights end to end against the numpy restatement of regress.jl (tests/_regress_np.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _regress_np as rn  # noqa: E402

pytestmark = pytest.mark.gpu

TASK_W = [0.05, 0.2, 0.3, 0.25]


# ---------------------------------------------------------------- rsys_op_target_rank against numpy
def _key(x):
    x = np.asarray(x, np.float32)
    u = np.where(x == 0, np.float32(0), x).astype(np.float32).view(np.uint32).astype(np.int64)
    k = np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(x) | (x == -np.inf), 0, k)


def _expect_rank(scores, targets):
    """1 + #{adm: s_i > s_t} + #{adm, i < t: s_i == s_t}, 0 when s_t is NaN or -inf (per row)"""
    k = _key(scores)
    kt = k[np.arange(k.shape[0]), targets][:, None]
    i = np.arange(k.shape[1])[None, :]
    r = 1 + np.sum(k > kt, 1) + np.sum((k == kt) & (i < np.asarray(targets)[:, None]), 1)
    return np.where(kt[:, 0] == 0, 0, r).astype(np.int32)


def _op_target_rank(scores, targets, ld=None):
    from recommendersystem_amd._lib import check, lib
    rows, V = scores.shape
    ld = V if ld is None else ld
    host = np.full((rows, ld), np.nan, np.float32)
    host[:, :V] = scores
    t = np.ascontiguousarray(targets, np.int32)
    L = lib()
    ptrs = []
    try:
        for nbytes in (host.nbytes, rows * 4, rows * 4):
            p = C.c_void_p()
            check(L.rsys_dev_alloc(C.byref(p), nbytes))
            ptrs.append(p)
        check(L.rsys_dev_h2d(ptrs[0], host.ctypes.data, host.nbytes))
        check(L.rsys_dev_h2d(ptrs[1], t.ctypes.data, t.nbytes))
        check(L.rsys_op_target_rank(ptrs[0], ld, rows, V, ptrs[1], ptrs[2]))
        out = np.empty(rows, np.int32)
        check(L.rsys_dev_d2h(out.ctypes.data, ptrs[2], out.nbytes))
    finally:
        for p in ptrs:
            L.rsys_dev_free(p)
    return out


def _rows(kind, rows, V, rng):
    if kind == "random":
        return rng.standard_normal((rows, V)).astype(np.float32) * 4 - 10
    if kind == "equal":
        return np.full((rows, V), -3.25, np.float32)
    if kind == "ulp":      # a handful of neighbouring floats: long runs of ties
        base = np.float32(-7.5).view(np.int32)
        return (base + rng.integers(0, 5, (rows, V))).astype(np.int32).view(np.float32)
    if kind == "zeros":    # +-0.0 mixed with a few values around them
        x = np.where(rng.random((rows, V)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        x[rng.random((rows, V)) < 0.05] = 1e-30
        x[rng.random((rows, V)) < 0.05] = -1e-30
        return x
    if kind == "special":  # -inf and NaN sprinkled in; the last row all -inf
        x = rng.standard_normal((rows, V)).astype(np.float32)
        x[rng.random((rows, V)) < 0.3] = -np.inf
        x[rng.random((rows, V)) < 0.1] = np.nan
        x[rng.random((rows, V)) < 0.01] = np.inf
        x[-1] = -np.inf
        return x
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["random", "equal", "ulp", "zeros", "special"])
@pytest.mark.parametrize("V,rows", [(119999, 8), (37, 64), (4096, 3), (4097, 5)])
def test_op_target_rank_bit_exact(kind, V, rows):
    rng = np.random.default_rng(V + rows)
    x = _rows(kind, rows, V, rng)
    t = rng.integers(0, V, rows).astype(np.int32)
    t[0] = V - 1
    got = _op_target_rank(x, t)
    assert np.array_equal(got, _expect_rank(x, t))
    for ld in (V + 3, V + (8 - V % 4)):                    # a row stride that breaks the 16-byte loads, and one that keeps them
        assert np.array_equal(_op_target_rank(x, t, ld), _expect_rank(x, t))


def test_op_target_rank_inadmissible_targets_and_many_rows():
    rng = np.random.default_rng(7)
    x = rng.integers(-4, 4, (3000, 300)).astype(np.float32)
    x[rng.random(x.shape) < 0.1] = -np.inf
    x[rng.random(x.shape) < 0.05] = np.nan
    t = rng.integers(0, 300, 3000).astype(np.int32)
    x[0, t[0]] = np.nan
    x[1, t[1]] = -np.inf
    got = _op_target_rank(x, t)
    assert got[0] == 0 and got[1] == 0
    assert np.array_equal(got, _expect_rank(x, t))


def test_op_target_rank_argument_errors():
    import recommendersystem_amd as ra
    x = np.zeros((2, 10), np.float32)
    for t, ld in (([0, 10], None), ([-1, 0], None)):
        with pytest.raises(ra.RsysError):
            _op_target_rank(x, t, ld)
    from recommendersystem_amd._lib import lib
    assert lib().rsys_op_target_rank(None, 10, 2, 10, None, None) != 0


# ---------------------------------------------------------------- the whole call
def _model(dtype, vocab=None, seed=9, deterministic=False, inference=False):
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config("hd64", mask_rate=0.2, mask_topk=16)
    if vocab:
        cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"] = vocab
    if deterministic:
        cfg["deterministic"] = True
    if inference:
        cfg["forward"] = "inference"
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=4)
    if vocab:
        model.init_weights(seed)
        model.random_pretrained_embeddings(seed + 1)
    else:
        model.load_state_dict(synth.make_params(cfg, seed, "test"))
    return cfg, model


def _queries(cfg, model, n, seed):
    """n retrieval embeddings: inference_select at random tokens of a synthetic batch, then random mixes of them"""
    from oracle import synth
    rows = 4
    S = cfg["max_sequence_length"]
    d = synth.make_batch(cfg, rows, seed)
    d["rope_input_pos"] = np.tile(np.arange(S, dtype=np.int32), rows)
    rng = np.random.default_rng(seed)
    base = model.inference_select(d, "retrieval", rng.choice(rows * 2 * S, size=16, replace=False).astype(np.int32))
    w = rng.standard_normal((n, base.shape[0])).astype(np.float32) / 3
    return (w @ base + 0.2 * rng.standard_normal((n, base.shape[1]))).astype(np.float32)


def _bf16(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16
    return b.astype(np.uint32).view(np.float32)


def _lp64(model, cfg, dtype, q, medium):
    n0 = cfg["vocab_sizes"]["0_matchedid"]
    F = model.item_embeddings()
    F = F[:n0] if medium == 0 else F[n0:]
    if dtype == "bf16":
        F, q = _bf16(F), _bf16(q)
    z = q.astype(np.float64) @ F.astype(np.float64).T
    zmax = z.max(1, keepdims=True)
    return z - (zmax + np.log(np.exp(z - zmax).sum(1, keepdims=True)))


def _check_fp64(rank, logp, lp, targets, exclude, tol_rel):
    """logp within tolerance of the fp64 value; the rank between the exact ranks of the target moved up and down by twice the
    tolerance, so equal to the exact rank wherever the target is separated from every other item by more than that.  Returns the
    number of users whose rank was pinned exactly."""
    n, V = lp.shape
    exact = 0
    for j in range(n):
        t = int(targets[j])
        tol = tol_rel * max(1.0, abs(lp[j, t]))
        assert abs(logp[j] - lp[j, t]) <= tol, (j, logp[j], lp[j, t])
        adm = np.ones(V, bool)
        adm[np.asarray(exclude[j], np.int64)] = False
        if not adm[t]:
            assert rank[j] == 0, j
            continue
        adm[t] = False
        o = lp[j, adm]
        lo, hi = 1 + np.sum(o > lp[j, t] + 2 * tol), 1 + np.sum(o >= lp[j, t] - 2 * tol)
        assert lo <= rank[j] <= hi, (j, rank[j], lo, hi)
        exact += int(lo == hi)
    return exact


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_target_rank_against_topk_and_fp64(dtype):
    cfg, model = _model(dtype, vocab=(60000, 40000))
    tol_rel = 2e-5 if dtype == "fp32" else 2e-3
    rng = np.random.default_rng(11)
    n = 40
    q = _queries(cfg, model, n, 3)
    for medium in (0, 1):
        Vm = cfg["vocab_sizes"][f"{medium}_matchedid"]
        exclude = [np.concatenate([[0], rng.integers(0, Vm, int(rng.integers(0, 300)))]) for _ in range(n)]
        for k in (1024, 8192):
            ids, sc, cnt = model.retrieve_topk(q, medium, k, exclude=exclude)
            # targets: list positions 1, k, a middle one, the last admissible one; ids past the list; an excluded one
            t = np.empty(n, np.int32)
            for j in range(n):
                c = int(cnt[j])
                kind = j % 6
                if kind < 3:
                    t[j] = ids[j, [0, c - 1, c // 2][kind]]
                elif kind == 3:
                    t[j] = rng.integers(0, Vm)
                elif kind == 4:
                    rest = np.setdiff1d(np.arange(Vm), ids[j, :c])
                    t[j] = rest[rng.integers(0, rest.size)]
                else:
                    t[j] = exclude[j][-1]
            rank, logp = model.retrieve_target_rank(q, medium, t, exclude=exclude)
            excl_t = np.array([t[j] in set(exclude[j].tolist()) for j in range(n)])
            assert (rank[excl_t] == 0).all() and (rank[~excl_t] >= 1).all()
            for j in range(n):
                c = int(cnt[j])
                pos = np.flatnonzero(ids[j, :c] == t[j])
                if 1 <= rank[j] <= k:
                    assert pos.size == 1 and pos[0] == rank[j] - 1, (j, rank[j], pos)
                    assert logp[j].view(np.uint32) == sc[j, rank[j] - 1].view(np.uint32) or (logp[j] == 0 and sc[j, rank[j] - 1] == 0)
                else:
                    assert pos.size == 0, (j, rank[j], pos)
                    if rank[j] > k:
                        assert c == k and logp[j] <= sc[j, c - 1]
        lp = _lp64(model, cfg, dtype, q, medium)
        _check_fp64(rank, logp, lp, t, exclude, tol_rel)
    model.close()


def test_chunking_and_the_python_split():
    cfg, model = _model("fp32")
    rng = np.random.default_rng(5)
    D = cfg["embed_dim"]
    for medium in (0, 1):
        Vm = cfg["vocab_sizes"][f"{medium}_matchedid"]
        for n in (255, 256, 257, 4096):
            q = (rng.standard_normal((n, D)) * 0.3).astype(np.float32)
            t = rng.integers(0, Vm, n).astype(np.int32)
            exclude = [rng.integers(0, Vm, int(rng.integers(0, 6))) for _ in range(n)]
            for j in range(0, n, 7):
                exclude[j] = np.append(exclude[j], t[j])             # the target excluded in every chunk
            rank, logp = model.retrieve_target_rank(q, medium, t, exclude=exclude)
            assert (rank[::7] == 0).all()
            lp = _lp64(model, cfg, "fp32", q, medium)
            assert _check_fp64(rank, logp, lp, t, exclude, 2e-5) >= 1
        n = 4100
        q = (rng.standard_normal((n, D)) * 0.3).astype(np.float32)
        t = rng.integers(0, Vm, n).astype(np.int32)
        exclude = [[0, int(t[j])] if j % 9 == 0 else [0] for j in range(n)]
        rank, logp = model.retrieve_target_rank(q, medium, t, exclude=exclude)
        r0, l0 = model.retrieve_target_rank(q[:4096], medium, t[:4096], exclude=exclude[:4096])
        r1, l1 = model.retrieve_target_rank(q[4096:], medium, t[4096:], exclude=exclude[4096:])
        assert np.array_equal(rank, np.concatenate([r0, r1])) and np.array_equal(logp.view(np.uint32), np.concatenate([l0, l1]).view(np.uint32))
    model.close()


def test_reproducible_and_follows_the_table():
    cfg, model = _model("bf16")
    rng = np.random.default_rng(8)
    q = _queries(cfg, model, 300, 6)
    t = rng.integers(0, 200, 300).astype(np.int32)
    a = model.retrieve_target_rank(q, 1, t)
    b = model.retrieve_target_rank(q, 1, t)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    name = "item_embedding.projection_layer.bias"
    bias = model.get_parameter(name)
    model.set_parameter(name, bias + rng.standard_normal(bias.shape).astype(np.float32))
    c = model.retrieve_target_rank(q, 1, t)
    assert c[1].tobytes() != a[1].tobytes()                          # the fused table was rebuilt
    model.set_parameter(name, bias)
    d = model.retrieve_target_rank(q, 1, t)
    assert a[0].tobytes() == d[0].tobytes() and a[1].tobytes() == d[1].tobytes()
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_eval_between_training_steps_changes_nothing(dtype):
    """Deterministic mode: step -> eval -> step gives the losses, gradients and parameters of step -> step, bit for bit."""
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config("hd64", mask_rate=0.2, deterministic=True)
    P = synth.make_params(cfg, 3, "test")
    rows = 4
    batches = [synth.make_batch(cfg, rows, 40 + i) for i in range(2)]
    masks = [synth.make_masks(cfg, rows, 50 + i) for i in range(2)]
    q = np.random.default_rng(0).standard_normal((3, cfg["embed_dim"])).astype(np.float32)
    names = synth.trainable_names(cfg)

    def run(evaluate):
        model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
        model.load_state_dict(P)
        opt = ra.create_optimizer(model, dict(cfg, learning_rate=1e-2))
        model.set_loss_weights(TASK_W, 1)
        out = []
        for i, (d, mk) in enumerate(zip(batches, masks)):
            if i == 1 and evaluate:
                model.retrieve_target_rank(q, 0, [1, 2, 3], exclude=[[0], [], [3]])
                model.retrieve_target_rank(q, 1, [5, 6, 7])
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
    from recommendersystem_amd._lib import lib
    cfg, model = _model("fp32")
    D = cfg["embed_dim"]
    q = np.zeros((2, D), np.float32)
    bad = [
        dict(queries=q, medium=2, targets=[1, 2]),
        dict(queries=q, medium=0, targets=[1, 120]),                  # V_0 = 120
        dict(queries=q, medium=1, targets=[-1, 2]),
        dict(queries=q, medium=0, targets=[1, 2], exclude=[[120], []]),
        dict(queries=q, medium=1, targets=[1, 2], exclude=[[-1], []]),
    ]
    for kw in bad:
        with pytest.raises(ra.RsysError):
            model.retrieve_target_rank(**kw)
    t = np.array([1, 2], np.int32)
    rank = np.empty(2, np.int32); logp = np.empty(2, np.float32)
    off = np.array([0, 2, 1], np.int64); ids = np.array([3, 4], np.int32)  # decreasing offsets
    assert lib().rsys_retrieve_target_rank(model._h, 0, q.ctypes.data, 2, t.ctypes.data, off.ctypes.data, ids.ctypes.data,
                                           rank.ctypes.data, logp.ctypes.data) != 0
    off = np.array([1, 1, 2], np.int64)
    assert lib().rsys_retrieve_target_rank(model._h, 0, q.ctypes.data, 2, t.ctypes.data, off.ctypes.data, ids.ctypes.data,
                                           rank.ctypes.data, logp.ctypes.data) != 0
    assert lib().rsys_retrieve_target_rank(model._h, 0, q.ctypes.data, 2, t.ctypes.data, off.ctypes.data, None,
                                           rank.ctypes.data, logp.ctypes.data) != 0
    big = np.zeros((4097, D), np.float32); tb = np.ones(4097, np.int32)
    rb = np.empty(4097, np.int32); lb = np.empty(4097, np.float32)
    assert lib().rsys_retrieve_target_rank(model._h, 0, big.ctypes.data, 4097, tb.ctypes.data, None, None, rb.ctypes.data, lb.ctypes.data) != 0
    assert lib().rsys_retrieve_target_rank(model._h, 0, q.ctypes.data, 0, t.ctypes.data, None, None, rank.ctypes.data, logp.ctypes.data) != 0
    r, lp = model.retrieve_target_rank(q, 0, [1, 2])                  # still usable
    assert r.tolist() == [2, 3]                                        # all scores equal: ties by id, item 0 first
    model.close()


# ---------------------------------------------------------------- regress.save_weights end to end
def _history(rng, V, n):
    items, ts = [], 1.2e9
    for _ in range(n):
        ts += float(rng.integers(10, 10 ** 6))
        y = int(rng.integers(0, 2))
        items.append({"medium": y, "matchedid": int(rng.integers(1, V[y])), "history_max_ts": ts, "status": int(rng.integers(0, 9)),
                      "rating": float(rng.integers(0, 11)), "progress": float(rng.random()), "history_status": -1, "history_rating": -1.0})
    return items, ts


def _test_users(rng, V, n):
    users = []
    for j in range(n):
        m = j % 2
        items, ts = _history(rng, V, int(rng.integers(3, 20)))
        held = {"medium": m, "matchedid": int(rng.integers(1, V[m])), "history_max_ts": ts + 60.0, "status": int(rng.choice([0, 6, 7, 8])),
                "rating": float(rng.integers(0, 11)), "progress": 1.0, "history_status": None, "history_rating": 0.0}
        users.append({"user": {"gender": None, "source": 2}, "items": items, "test_items": [held]})
    return users


def test_save_weights_end_to_end_and_coefficients_reach_serving():
    from recommendersystem_amd import regress, serve
    cfg, model = _model("fp32", seed=31, inference=True)
    V = (cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"])
    n0 = V[0]
    embs = model.item_embeddings()
    mean = np.float32(cfg["rating_mean"]) if "rating_mean" in cfg else np.float32(0.0)
    registry = {"0.watch.weight": embs[:n0], "1.watch.weight": embs[n0:], "0.rating_mean": mean, "1.rating_mean": mean}
    rng = np.random.default_rng(12)
    users = _test_users(rng, V, 24)
    K = 64
    out = regress.save_weights(model, users, registry, num_ranking_items=K)
    for m in (0, 1):
        recs = regress.regress_records(model, users, m, num_ranking_items=K)
        assert recs and all(r["matchedid"] in r["ranking_matchedids"].tolist() for r in recs)
        lp_full = [rn_lp(registry, m, r) for r in recs]
        # retrieval metrics: the restatement on the records whose target has no near tie (the device ranks in fp32)
        sep = [i for i, (r, row) in enumerate(zip(recs, lp_full)) if _separated(row, r["matchedid"], 1e-4)]
        sub = [recs[i] for i in sep]
        want = rn.retrieval_metrics(sub, [lp_full[i] for i in sep], m)
        got = regress.retrieval_metrics(model, sub, m)
        for k in want:
            assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-15), k
        ce = rn.regress_retrieval(recs, [row[r["matchedid"]] for row, r in zip(lp_full, recs)], m)
        assert out[f"{m}.retrieval.crossentropy"] == pytest.approx(ce[f"{m}.retrieval.crossentropy"], rel=1e-4)
        assert out[f"{m}.retrieval.num_users"] == ce[f"{m}.retrieval.num_users"]
        fit = rn.regress_ranking(recs, registry, m)
        np.testing.assert_allclose(out[f"{m}.rating.coefs"], fit[f"{m}.rating.coefs"], rtol=1e-6, atol=1e-9)
        # ranking metrics with the fitted coefficients, on the records whose candidate scores have no near tie at the target
        c = np.asarray(out[f"{m}.rating.coefs"], np.float32)
        lp = [row[r["ranking_matchedids"]].astype(np.float32) for row, r in zip(lp_full, recs)]
        rr_ = [np.float32(c[0]) * np.float32(mean) + np.float32(c[1]) * r[f"{m}.ranking"] for r in recs]
        sep = [i for i, r in enumerate(recs) if _separated(lp[i] + rr_[i], list(r["ranking_matchedids"]).index(r["matchedid"]), 1e-3)
               and _separated(lp[i], list(r["ranking_matchedids"]).index(r["matchedid"]), 1e-3)]
        sub = [recs[i] for i in sep]
        if any(not regress.skip_user(r, m, "retrieval") for r in sub):
            want = rn.ranking_metrics(sub, [lp[i] for i in sep], [rr_[i] for i in sep], m)
            got = regress.ranking_metrics(model, sub, out, m)
            for k in want:
                assert got[k] == pytest.approx(want[k], rel=1e-6), k
        for k in ("HR", "nDCG"):
            assert 0.0 <= out[f"{m}.retrieval.{k}@1024"] <= 1.0
        # the fitted coefficients reach serve.ranking: score = log p + c0 * rating_mean + c1 * r_masked
        r0 = recs[0]
        st = dict(medium=m, users=[{"user": {"items": []}, "embeds": {f"{m}.retrieval": r0[f"{m}.retrieval"], f"{m}.ranking": r0[f"{m}.ranking"]}}])
        got = serve.ranking(model, [st], [r0["ranking_matchedids"]], out)[0]
        want = lp_full[0][r0["ranking_matchedids"]] + c[0] * mean + c[1] * r0[f"{m}.ranking"].astype(np.float64)
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)
        plain = serve.ranking(model, [st], [r0["ranking_matchedids"]], registry)[0]
        assert not np.allclose(plain, got)
    model.close()


def rn_lp(registry, m, r):
    z = np.asarray(registry[f"{m}.watch.weight"], np.float64) @ np.asarray(r[f"{m}.retrieval"], np.float64)
    zmax = z.max()
    return z - (zmax + np.log(np.exp(z - zmax).sum()))


def _separated(row, t, tol):
    row = np.asarray(row, np.float64)
    d = np.abs(np.delete(row, t) - row[t])
    return d.size == 0 or np.min(d) > tol * max(1.0, abs(row[t]))
