"""GPU: the item-similarity LambdaRank model on the device (rsys_sim_*, recommendersystem_amd/similarity.py; pairwise_ltr.py) against the
float64 restatement in tests/_similarity_np.py: ranks, loss and gradients in both dtypes, dropout, nDCG, AdamW with the skip on a non-finite
gradient, the export, hard negatives bit for bit, reproducibility, argument errors, a short training run, one step at the reference
shape, and the tables of models fed from a transformer's item table driving rsys_retrieve_request."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _similarity_np as sn  # noqa: E402

pytestmark = pytest.mark.gpu

V, F, E, NQ, N = 3000, 256, 128, 8, 128


def _model(dtype="fp32", dropout=0.0, seed=0, n=N, nq=NQ, v=V, f=F, e=E, feat=None):
    from recommendersystem_amd import similarity as sim
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((v, f)).astype(np.float32) if feat is None else feat
    cfg = sim.training_config({0: v}, embed_dim=e, batch_size=nq, items_per_query=n)
    m = sim.LTRModel(cfg, 0, feat, dtype=dtype, dropout=dropout)
    W = (rng.standard_normal((e, f)) / np.sqrt(f)).astype(np.float32)
    m.param_set("encoder.1.weight", W)
    return m, feat, W


def _batch(seed=1, nq=NQ, n=N, v=V, ties=False):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, v, nq)
    tgt = rng.integers(0, v, (nq, n))
    rel = np.where(rng.random((nq, n)) < 0.3, rng.integers(1, 6, (nq, n)).astype(np.float64), 0.0)
    if ties:   # repeated targets give repeated scores; equal relevances everywhere
        tgt[:, 1::2] = tgt[:, 0::2]
    w = np.sqrt(rng.integers(1, 100, nq).astype(np.float64))
    return {"sourceid": np.repeat(src[:, None], n, 1), "targetid": tgt, "relevance": rel, "weight": w[:, None]}


def _relerr(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-30))


def test_ranks_with_ties():
    m, feat, W = _model()
    b = _batch(ties=True)
    m.forward_backward(b, evaluate=True)
    x = m.debug("scores", (NQ, N), np.float32)
    r = m.debug("ranks", (NQ, N), np.int32)
    assert np.any(x[:, 0::2] == x[:, 1::2])
    np.testing.assert_array_equal(r, sn.ranks(x))


def test_loss_and_gradients_fp32():
    m, feat, W = _model()
    b = _batch()
    ls = m.get_temperature()
    m.zero_grad()
    loss = m.forward_backward(b)
    src = b["sourceid"][:, 0]
    ref_loss, x, g, dW, dls = sn.forward_backward(feat, W, ls, src, b["targetid"], b["relevance"], b["weight"][:, 0])
    assert abs(loss - ref_loss) / abs(ref_loss) < 1e-4
    assert _relerr(m.debug("dldx", (NQ, N), np.float32), g) < 1e-4
    assert _relerr(m.param_get("encoder.1.weight", grad=True), dW) < 1e-4
    assert abs(float(m.param_get("logit_scale", grad=True)) - dls) <= 1e-4 * max(abs(dls), 1e-3)


def test_loss_and_gradients_bf16():
    # the oracle rounds the same operands (features, W, the encoder output, dY) to bf16 and takes the device's ranks, so no tie can flip;
    # what remains is the fp32 accumulation order and the rare bf16 rounding it moves across a boundary.  Leaving out the rounding of dY
    # alone moves dW by 4e-3 at this shape, computing in fp32 moves dL/dx by 9e-3: the bounds below see either.
    m, feat, W = _model("bf16")
    b = _batch()
    ls = m.get_temperature()
    m.zero_grad()
    loss = m.forward_backward(b)
    order = m.debug("ranks", (NQ, N), np.int32)
    ref_loss, x, g, dW, dls = sn.forward_backward_by_id(feat, W, ls, b["sourceid"][:, 0], b["targetid"], b["relevance"],
                                                        b["weight"][:, 0], order, bf16_mode=True)
    _check_grads(m, loss, ref_loss, g, dW, dls, NQ, N, tol_loss=1e-4, tol=1e-3)


def _check_grads(m, loss, ref_loss, g, dW, dls, nq, n, tol_loss, tol):
    assert abs(loss - ref_loss) / abs(ref_loss) < tol_loss, (loss, ref_loss)
    e = _relerr(m.debug("dldx", (nq, n), np.float32), g)
    assert e < tol, ("dldx", e)
    e = _relerr(m.param_get("encoder.1.weight", grad=True), dW)
    assert e < tol, ("dW", e)
    gl = float(m.param_get("logit_scale", grad=True))
    assert abs(gl - dls) <= tol * max(abs(dls), 1e-3), ("dls", gl, dls)


def test_reference_shaped_step_bf16():
    """one step at pairwise_ltr.py's shape (n_q 128, n 2048, F 2048, E 1024, bf16): eight pair-loss workgroups per list, the 2048-slot
    rank sort, the K-major split-K dW (K = 524 288) summed in split order; against the oracle fed the device's ranks, then bitwise
    reproducibility of a step with dropout"""
    nq, n, f, e, v = 128, 2048, 2048, 1024, 8192
    m, feat, W = _model("bf16", dropout=0.0, nq=nq, n=n, v=v, f=f, e=e)
    rng = np.random.default_rng(11)
    src = rng.integers(0, v, nq)
    rel = np.zeros((nq, n))
    npos = int(n * 0.9)
    rel[:, :npos] = rng.integers(1, 50, (nq, npos))
    b = {"sourceid": np.repeat(src[:, None], n, 1), "targetid": rng.integers(0, v, (nq, n)), "relevance": rel,
         "weight": np.sqrt(rng.integers(1, 1000, (nq, 1)).astype(np.float64))}
    ls = m.get_temperature()
    m.zero_grad()
    loss = m.forward_backward(b)
    order = m.debug("ranks", (nq, n), np.int32)
    ref_loss, x, g, dW, dls = sn.forward_backward_by_id(feat, W, ls, src, b["targetid"], rel, b["weight"][:, 0], order, bf16_mode=True)
    _check_grads(m, loss, ref_loss, g, dW, dls, nq, n, tol_loss=1e-4, tol=1e-3)
    m.close()
    m, _, _ = _model("bf16", dropout=0.1, nq=nq, n=n, v=v, f=f, e=e)
    outs = []
    for _ in range(2):
        m.zero_grad()
        loss = m.forward_backward(b, seed=5, step=9)
        outs.append((loss, m.param_get("encoder.1.weight", grad=True), m.param_get("logit_scale", grad=True)))
    assert outs[0][0] == outs[1][0]
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    np.testing.assert_array_equal(outs[0][2], outs[1][2])
    assert np.isfinite(outs[0][1]).all() and np.abs(outs[0][1]).max() > 0


def test_dropout_masks():
    p = 0.1
    m, feat, W = _model(dropout=p)
    b = _batch()
    ls = m.get_temperature()
    m.zero_grad()
    loss = m.forward_backward(b, seed=7, step=3)
    mask = m.debug("dropout_mask", (2 * NQ * N, F), np.uint8).astype(bool)
    assert 0.85 < mask.mean() < 0.95
    ms, mt = mask[:NQ * N], mask[NQ * N:]
    assert not np.array_equal(ms[0], ms[1])          # the copies of one source differ
    ref_loss, x, g, dW, dls = sn.forward_backward(feat, W, ls, b["sourceid"][:, 0], b["targetid"], b["relevance"], b["weight"][:, 0],
                                                  masks=(ms, mt), p=p)
    assert abs(loss - ref_loss) / abs(ref_loss) < 1e-4
    assert _relerr(m.param_get("encoder.1.weight", grad=True), dW) < 1e-4


def test_ndcg_with_ties():
    for dtype, tol in (("fp32", 1e-5), ("bf16", 1e-2)):
        m, feat, W = _model(dtype)
        b = _batch(ties=True)
        s, w = m.ndcg(b)
        x = m.debug("scores", (NQ, N), np.float32)
        rs, rw = sn.ndcg(x, b["relevance"], b["weight"][:, 0].astype(np.float32))   # (the device takes f32 weights)
        assert abs(w - rw) < 1e-9 * rw
        assert abs(s - rs) < 1e-5 * rw
        xr = sn.scores_eval(feat, W, m.get_temperature(), b["sourceid"][:, 0], b["targetid"], bf16_mode=dtype == "bf16")
        assert _relerr(x, xr) < tol


def test_adamw_and_skip():
    m, feat, W = _model()
    ls0 = m.get_temperature()
    p = [W.astype(np.float64), np.array(ls0)]
    mm = [np.zeros_like(p[0]), np.zeros(())]
    vv = [np.zeros_like(p[0]), np.zeros(())]
    for step in range(1, 4):
        b = _batch(seed=10 + step)
        m.zero_grad()
        m.forward_backward(b)
        g = [m.param_get("encoder.1.weight", grad=True).astype(np.float64), m.param_get("logit_scale", grad=True).astype(np.float64)]
        norm, skipped = m.adamw_step(3e-4, 1.0)
        out, rnorm = sn.adamw(p, g, mm, vv, step, 3e-4, [0.1, 0.0], 1.0)
        p = [o[0] for o in out]; mm = [o[1] for o in out]; vv = [o[2] for o in out]
        assert not skipped and abs(norm - rnorm) < 1e-4 * rnorm
    assert _relerr(m.param_get("encoder.1.weight"), p[0]) < 1e-5
    assert abs(m.get_temperature() - float(p[1])) < 1e-5
    # a non-finite gradient skips the step: parameters, moments and the step count stay
    from recommendersystem_amd._lib import check, lib
    W1, ls1 = m.param_get("encoder.1.weight"), m.get_temperature()
    m1, v1, st1 = m.adamw_state("encoder.1.weight")
    assert st1 == 3
    bad = feat.copy()
    bad[5] = np.inf
    check(lib().rsys_sim_features_set(m.h, bad.ctypes.data_as(C.c_void_p), V, F))
    b = _batch(seed=20)
    b["targetid"][0, 0] = 5
    m.zero_grad()
    m.forward_backward(b)
    norm, skipped = m.adamw_step(3e-4, 1.0)
    assert skipped and not np.isfinite(norm)
    np.testing.assert_array_equal(m.param_get("encoder.1.weight"), W1)
    assert m.get_temperature() == ls1
    m2, v2, st2 = m.adamw_state("encoder.1.weight")
    assert st2 == 3
    np.testing.assert_array_equal(m2, m1)
    np.testing.assert_array_equal(v2, v1)


def test_export_both_modes():
    for dtype in ("fp32", "bf16"):
        m, feat, W = _model(dtype, dropout=0.1)
        e = m.embed_all(train_mode=False)
        ref = sn.normalize(feat.astype(np.float64) @ W.astype(np.float64).T)
        assert _relerr(e, ref) < 1e-5
        e1 = m.embed_all(train_mode=True, seed=3)
        e2 = m.embed_all(train_mode=True, seed=3)
        np.testing.assert_array_equal(e1, e2)
        assert _relerr(e1, ref) > 1e-3


def test_hard_negatives_bit_exact():
    # integer embeddings: every dot product is exact in fp32, so the bf16-rounded scores are known exactly (and tie a lot)
    rng = np.random.default_rng(5)
    v = 700
    m, _, _ = _model(v=v, n=256)
    emb = rng.integers(-3, 4, (v, E)).astype(np.float32)
    emb[10:20] = emb[9]
    m.set_export(emb)
    tm = rng.random((v, v)) < 0.02
    tm[:, 600:] = True            # the test split of the sources below sees few admissible ids: the -inf fill
    m.set_testmask(tm)
    # three chunks of 256 sources: the chunk offsets of the output and of the positive lists
    sources = np.concatenate([[0, 9, 15, 600, 699, 9], rng.integers(0, v, 594)])
    positives = [rng.integers(0, v, k).tolist() for k in (0, 5, 30, 3, 0, 1)] + [rng.integers(0, v, k).tolist()
                                                                                  for k in rng.integers(0, 40, 594)]
    sc = sn.bf16(emb.astype(np.float64) @ emb.astype(np.float64).T)
    for split, n in (("training", 256), ("test", 200)):
        out = m.hard_negatives(split, sources, positives, n)
        for i, s in enumerate(sources):
            ref = sn.hard_negatives(sc[s], s, tm[s], split, positives[i], n)
            np.testing.assert_array_equal(out[i], ref)


def test_reproducible():
    outs = []
    for _ in range(2):
        m, feat, W = _model("bf16", dropout=0.1)
        b = _batch()
        m.zero_grad()
        loss = m.forward_backward(b, seed=1, step=2)
        outs.append((loss, m.param_get("encoder.1.weight", grad=True), m.param_get("logit_scale", grad=True)))
        m.close()
    assert outs[0][0] == outs[1][0]
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    np.testing.assert_array_equal(outs[0][2], outs[1][2])


def test_argument_errors():
    from recommendersystem_amd import RsysError, similarity as sim
    from recommendersystem_amd._lib import lib
    m, feat, W = _model()
    b = _batch()
    b["targetid"][0, 0] = V
    with pytest.raises(RsysError):
        m.forward_backward(b)
    b = _batch(n=N)
    big = {k: np.concatenate([v, v], axis=1) if v.ndim == 2 and v.shape[1] == N else v for k, v in b.items()}
    with pytest.raises(RsysError):
        m.forward_backward(big)
    with pytest.raises(RsysError):
        check_wrong_f = lib().rsys_sim_features_set(m.h, feat.ctypes.data_as(C.c_void_p), V, F + 64)
        sim.check(check_wrong_f)
    m.set_export(np.zeros((V, E), np.float32))
    m.set_testmask(np.zeros((V, V), bool))
    with pytest.raises(RsysError):
        m.hard_negatives("training", [0], [[V + 1]], 10)
    off = np.array([0, 2, 1], np.int64)
    out = np.zeros((2, 10), np.int32)
    src = np.array([0, 1], np.int32)
    pid = np.array([1, 2], np.int32)
    with pytest.raises(RsysError):
        sim.check(lib().rsys_sim_hard_negatives(m.h, 0, 2, src.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                                                pid.ctypes.data_as(C.c_void_p), 10, out.ctypes.data_as(C.c_void_p)))
    with pytest.raises(RsysError):
        m.hard_negatives("training", [0], [[]], N + 1)
    with pytest.raises(RsysError):
        m.param_get("no.such.tensor")


def test_training_raises_ndcg(tmp_path):
    """a planted similarity: items come in clusters, pairs link items of one cluster with a score that falls with the distance inside it;
    30 epochs of similarity.train lift the test nDCG well above its initial value"""
    from recommendersystem_amd import similarity as sim
    rng = np.random.default_rng(3)
    v, f, e, n = 512, 64, 64, 32
    cl = rng.integers(0, 16, v)
    feat = (rng.standard_normal((v, f)) + 0.0).astype(np.float32)
    centers = rng.standard_normal((16, f)).astype(np.float32)
    feat = (0.7 * centers[cl] + feat).astype(np.float32)
    rows = {k: [] for k in ("cliptype", "source_matchedid", "source_popularity", "target_matchedid", "score")}
    for s in range(v):
        same = np.flatnonzero(cl == cl[s])
        same = same[same != s]
        for t in rng.choice(same, min(12, len(same)), replace=False):
            rows["cliptype"].append(0); rows["source_matchedid"].append(s); rows["source_popularity"].append(10.0)
            rows["target_matchedid"].append(int(t)); rows["score"].append(float(1.0 + (feat[s] @ feat[t]) / f))
    pairs = {k: np.array(x) for k, x in rows.items()}
    tm = rng.random((v, v)) < 0.25
    cfg = sim.training_config({0: v}, embed_dim=e, learning_rate=3e-3, batch_size=64, items_per_query=n)
    m = sim.LTRModel(cfg, 0, feat, dtype="bf16", dropout=0.1)
    m.param_set("encoder.1.weight", (rng.standard_normal((e, f)) / np.sqrt(f)).astype(np.float32))
    losses = []
    sim.train(m, pairs, tm, str(tmp_path), num_epochs=30, seed=1, log=losses.append)
    first = float(losses[0].split("Test Loss: ")[1])
    best = min(float(x.split("Test Loss: ")[1]) for x in losses)
    assert 1 - best > (1 - first) + 0.05, losses
    rows = open(tmp_path / "pairwise.model.0.csv").read().splitlines()
    assert rows[0] == "epoch,training_loss,test_loss,saved" and rows[1].startswith("-1,")
    ck = sim.load_checkpoint(str(tmp_path / "pairwise.model.0.npz"))
    assert ck["encoder.1.weight"].shape == (e, f) and "logit_scale" in ck


def test_tables_from_model_feed_retrieval_request():
    """end to end: both media's features straight from a transformer model's item table (rsys_sim_features_from_model), a training
    step, the eval-mode exports, item_similarity_tables, serve.load_retrieval_tables, and rsys_retrieve_request against the numpy
    restatement of render.jl (tests/_render_retrieval_np.py) with the prior of those tables"""
    import _render_retrieval_np as rr
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import serve, similarity as sim
    cfg = synth.make_config("hd64", mask_rate=0.2, mask_topk=16)
    cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"] = 3000, 2000
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=4)
    model.init_weights(9)
    model.random_pretrained_embeddings(10)
    V = (3000, 2000)
    D = cfg["embed_dim"]
    table = model.item_embeddings().astype(np.float64)
    rows = {0: table[:V[0]], 1: table[V[0]:]}
    rng = np.random.default_rng(21)
    emb = {}
    for m in (0, 1):
        scfg = sim.training_config({m: V[m]}, embed_dim=64, batch_size=4, items_per_query=64)
        s = sim.LTRModel(scfg, m, model, dtype="fp32", dropout=0.1)
        assert (s.V, s.F) == (V[m], D)
        W = (rng.standard_normal((64, D)) / np.sqrt(D)).astype(np.float32)
        s.param_set("encoder.1.weight", W)
        e0 = s.embed_all(train_mode=False)
        assert _relerr(e0, sn.normalize(rows[m] @ W.T.astype(np.float64))) < 1e-5   # the features are the model's rows of medium m
        src = rng.integers(0, V[m], 4)
        b = {"sourceid": np.repeat(src[:, None], 64, 1), "targetid": rng.integers(0, V[m], (4, 64)),
             "relevance": np.where(rng.random((4, 64)) < 0.3, 1.0, 0.0), "weight": np.ones((4, 1))}
        s.zero_grad()
        s.forward_backward(b)
        s.adamw_step(3e-4, 1.0)
        emb[m] = s.eval().embed_all()
        s.close()
    ad = {m: {"training": (rng.integers(0, V[m], 300), rng.integers(0, V[1 - m], 300)),
              "test": (rng.integers(0, V[m], 30), rng.integers(0, V[1 - m], 30))} for m in (0, 1)}
    tables, metrics = sim.item_similarity_tables(emb, ad)
    assert all(np.isfinite(v) for v in metrics.values())
    rel = rr.random_relations(rng, V, density=0.0005)
    released = {m: rng.random(V[m]) < 0.9 for m in (0, 1)}
    serve.load_retrieval_tables(model, rel, tables, released)
    n0 = V[0]
    F32 = model.item_embeddings()
    for m in (0, 1):
        states = [rr.random_state(rng, V, m, n_users=1 + j % 2, n_items=50, n_selected=1 + j % 4) for j in range(6)]
        for st in states:
            for u in st["users"]:
                u.setdefault("embeds", {f"{m}.retrieval": rng.standard_normal(D).astype(np.float32)})
        q, group, hist, sel = serve.request_arrays(states, m)
        k = 512
        ids, sc, cnt = model.retrieve_request(q, m, k, group=group, histories=hist, selected=sel)
        Fm = (F32[:n0] if m == 0 else F32[n0:]).astype(np.float64)
        z = Fm @ q.astype(np.float64).T
        zmax = z.max(0)
        lp = (z - (zmax + np.log(np.exp(z - zmax).sum(0)))).T
        ref = np.stack([rr.prior_fp64(m, tables, st, V) for st in states])
        for i, g in enumerate(group):
            ref[g] += lp[i]
        adm = np.stack([~rr.set_mask(m, rel, st, V, released=released[m]) for st in states])
        tol = 2e-5
        for gi in range(len(states)):
            nsel = int(cnt[gi])
            assert nsel == min(k, int(adm[gi].sum()))
            got = ids[gi, :nsel]
            assert adm[gi, got].all() and len(set(got.tolist())) == nsel
            assert (np.abs(sc[gi, :nsel] - ref[gi, got]) <= tol * np.maximum(1.0, np.abs(ref[gi, got]))).all()
            rest = adm[gi].copy(); rest[got] = False
            lo = sc[gi, nsel - 1]
            assert (ref[gi, rest] <= lo + 2 * tol * max(1.0, abs(lo))).all()
        # every group has selected items, so the tables' prior moves every score row
        assert all(np.abs(rr.prior_fp64(m, tables, st, V)).max() > 1e-3 for st in states)
    model.close()


def test_features_from_model_errors():
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import RsysError, similarity as sim
    from recommendersystem_amd._lib import lib
    cfg = synth.make_config("hd64", mask_rate=0.2, mask_topk=16)
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=4)
    V0 = cfg["vocab_sizes"]["0_matchedid"]
    s = sim.LTRModel(sim.training_config({0: V0 + 1}, embed_dim=64, batch_size=2, items_per_query=8), 0,
                     np.zeros((V0 + 1, cfg["embed_dim"]), np.float32), dtype="fp32")
    with pytest.raises(RsysError):
        sim.check(lib().rsys_sim_features_from_model(s.h, model._h, 0))     # V_0 differs from the handle's V
    with pytest.raises(RsysError):
        sim.check(lib().rsys_sim_features_from_model(s.h, model._h, 2))     # no medium 2
    s.close()
    model.close()
