"""GPU: the search model on the device (rsys_search_*, recommendersystem_amd/search.py; Training/search/train.py) against the float64
restatement in tests/_search_np.py: loss and gradients in both dtypes, argument errors, gradient accumulation, AdamW with the skip on a
non-finite gradient, reproducibility, the export, top-k serving, features from a transformer model, a short training run and one step
at the reference shape.

Test data: E_m ~ N(0, 1 / D), Wenc ~ N(0, a^2 / Q), x ~ N(0, 1), so a raw score P . E_i ~ N(0, a^2) and a logit ~ N(0, (a exp(s))^2).
`a` is chosen per logit_scale so that the logits' spread is known in advance (see _A): what fp32 can resolve of a soft-max
probability is ulp(logit), so a comparison at 1e-4 needs logits of at most a few hundred."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _search_np as sn  # noqa: E402

pytestmark = pytest.mark.gpu

V, D, Q = 3001, 128, 192
# fp32: logits of std 4 at s = 1 and std 30 at s = 5 (the largest of 3001 is then ~ 105 > 88.7 = log(FLT_MAX): without the row maximum
# subtracted the soft-max overflows).  bf16: a rounding of P that the accumulation order moves across a boundary shifts a logit by
# 2^-8 of its size, and the probability by as much in absolute terms, so the logits stay at std ~ 4 in both cases.
_A = {"fp32": {1.0: 1.5, 5.0: 0.2}, "bf16": {1.0: 1.5, 5.0: 0.03}}


def _model(dtype="fp32", s=1.0, seed=0, v=V, d=D, q=Q, max_batch=64, a=None):
    from recommendersystem_amd import search
    rng = np.random.default_rng(seed)
    feat = (rng.standard_normal((v, d)) / np.sqrt(d)).astype(np.float32)
    cfg = search.training_config({0: v}, batch_size=max_batch, embed_dim=d, query_dim=q)
    m = search.SearchModel(cfg, 0, feat, dtype=dtype, max_batch=max_batch)
    a = _A[dtype][s] if a is None else a
    W = (rng.standard_normal((q, d)) * a / np.sqrt(q)).astype(np.float32)
    m.param_set("encoder.weight", W)
    m.param_set("logit_scale", s)
    return m, feat, W


def _batch(B, seed=1, v=V, q=Q):
    rng = np.random.default_rng(seed)
    return {"queries": rng.standard_normal((B, q)).astype(np.float32), "matchedids": rng.integers(0, v, B),
            "mediums": np.zeros(B, np.int64), "weight": np.sqrt(rng.integers(1, 100, B).astype(np.float64))}


def _relerr(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-30))


def _check(m, b, ref, tol, tag):
    B = len(b["matchedids"])
    loss, wsum = m.last
    errs = {"loss": abs(loss - ref["loss"]) / abs(ref["loss"]),
            "lse": _relerr(m.debug("lse", (B,)), ref["lse"]),
            "dP": _relerr(m.debug("dP", (B, m.D)), ref["dP"]),
            "dWenc": _relerr(m.param_get("encoder.weight", grad=True), ref["dWenc"]),
            "ds": abs(float(m.param_get("logit_scale", grad=True)) - ref["ds"]) / max(abs(ref["ds"]), 1e-3)}
    print(tag, {k: f"{e:.2e}" for k, e in errs.items()})
    assert np.isfinite(loss)
    assert abs(wsum - ref["weight_sum"]) <= 1e-6 * ref["weight_sum"]
    for k, e in errs.items():
        assert e < tol, (tag, k, e)


@pytest.mark.parametrize("s", [1.0, 5.0])
@pytest.mark.parametrize("B", [37, 1])
def test_loss_and_gradients_fp32(B, s):
    m, feat, W = _model("fp32", s)
    b = _batch(B)
    m.zero_grad()
    m.last = m.forward_backward(b)
    ref = sn.forward_backward(feat, W, s, b["queries"], b["matchedids"], b["weight"])
    if s == 5.0:
        assert ref["z"].max() > 88.8   # the case does need the row maximum subtracted
    _check(m, b, ref, 1e-4, f"fp32 B={B} s={s}")


@pytest.mark.parametrize("s", [1.0, 5.0])
@pytest.mark.parametrize("B", [37, 1])
def test_loss_and_gradients_bf16(B, s):
    # the restatement rounds the operands the device rounds (x, Wenc, E_m, P, G and the dP that enters dWenc) and keeps everything else
    # in fp64; what remains is the fp32 accumulation order and the rare bf16 rounding it moves across a boundary.  On the restatement
    # itself at this shape (B = 37, s = 1), leaving out the rounding of P alone moves dWenc by 2.7e-3 and dP by 2.0e-3, leaving out
    # the rounding of G alone moves dWenc by 2.9e-3 and dP by 1.8e-3 (test_search_host.py asserts both): the 1e-3 below sees either.
    m, feat, W = _model("bf16", s)
    b = _batch(B)
    m.zero_grad()
    m.last = m.forward_backward(b)
    ref = sn.forward_backward(feat, W, s, b["queries"], b["matchedids"], b["weight"], bf16_mode=True)
    _check(m, b, ref, 1e-3, f"bf16 B={B} s={s}")


def test_argument_errors():
    from recommendersystem_amd import RsysError
    from recommendersystem_amd._lib import lib
    from recommendersystem_amd.search import _ptr
    import ctypes as C
    m, feat, W = _model("fp32", max_batch=8)
    good = _batch(4)

    def call(x, y, w, B):
        x = np.ascontiguousarray(x, np.float32); y = np.ascontiguousarray(y, np.int32); w = np.ascontiguousarray(w, np.float32)
        return lib().rsys_search_forward_backward(m.h, _ptr(x), _ptr(y), _ptr(w), B, 0, None, None)

    x, y, w = good["queries"], good["matchedids"], good["weight"]
    for bad_y in (np.array([0, 1, V, 2]), np.array([0, -1, 1, 2])):
        assert call(x, bad_y, w, 4) == -1
    assert call(x, y, np.zeros(4), 4) == -1
    assert call(x, y, np.array([1, -1, 1, 1.0]), 4) == -1
    assert call(x, y, np.array([1, np.nan, 1, 1.0]), 4) == -1
    assert call(x, y, np.array([1, np.inf, 1, 1.0]), 4) == -1
    assert call(x, y, w, 0) == -1
    big = _batch(9)
    assert call(big["queries"], big["matchedids"], big["weight"], 9) == -1
    ids, lp = np.zeros((1, V + 1), np.int32), np.zeros((1, V + 1), np.float32)
    assert lib().rsys_search_topk(m.h, _ptr(np.ascontiguousarray(x[:1])), 1, V + 1, _ptr(ids), _ptr(lp)) == -1
    assert lib().rsys_search_topk(m.h, _ptr(np.ascontiguousarray(x[:1])), 1, 0, _ptr(ids), _ptr(lp)) == -1
    xn = np.ascontiguousarray(x[:1]).copy(); xn[0, 3] = np.nan
    assert lib().rsys_search_topk(m.h, _ptr(xn), 1, 4, _ptr(ids), _ptr(lp)) == -1
    with pytest.raises(RsysError):
        m.debug("nope", (1,))
    norm = C.c_float(0)
    assert lib().rsys_search_adamw_step(m.h, 1e-3, 1.0, C.byref(norm), None) == -3   # no optimizer yet
    # the handle is still usable
    m.zero_grad()
    loss, _ = m.forward_backward(good)
    ref = sn.forward_backward(feat, W, 1.0, x, y, w)
    assert abs(loss - ref["loss"]) < 1e-4 * ref["loss"]


def test_evaluate_leaves_grad_and_calls_accumulate():
    m, feat, W = _model("fp32")
    b1, b2 = _batch(16, seed=3), _batch(16, seed=4)
    m.zero_grad()
    m.forward_backward(b1)
    g1, s1 = m.param_get("encoder.weight", grad=True), m.param_get("logit_scale", grad=True)
    l_eval, _ = m.forward_backward(b2, evaluate=True)
    np.testing.assert_array_equal(m.param_get("encoder.weight", grad=True), g1)
    np.testing.assert_array_equal(m.param_get("logit_scale", grad=True), s1)
    m.forward_backward(b2)
    r1 = sn.forward_backward(feat, W, 1.0, b1["queries"], b1["matchedids"], b1["weight"])
    r2 = sn.forward_backward(feat, W, 1.0, b2["queries"], b2["matchedids"], b2["weight"])
    assert abs(l_eval - r2["loss"]) < 1e-4 * r2["loss"]
    assert _relerr(m.param_get("encoder.weight", grad=True), r1["dWenc"] + r2["dWenc"]) < 1e-4
    assert abs(float(m.param_get("logit_scale", grad=True)) - (r1["ds"] + r2["ds"])) < 1e-4 * abs(r1["ds"] + r2["ds"])


def test_smaller_batch_after_a_larger_one():
    """rows of G an earlier, larger call wrote must not reach the next call's products"""
    m, feat, W = _model("bf16")
    m.zero_grad()
    m.forward_backward(_batch(37, seed=8))
    b = _batch(5, seed=9)
    m.zero_grad()
    m.last = m.forward_backward(b)
    ref = sn.forward_backward(feat, W, 1.0, b["queries"], b["matchedids"], b["weight"], bf16_mode=True)
    _check(m, b, ref, 1e-3, "bf16 B=5 after B=37")


def test_adamw_and_skip():
    """clip + three AdamW steps (torch's default betas, the two decay groups) against the restatement's AdamW fed the device's
    gradients (which test_loss_and_gradients_fp32 bounds), then a step on a non-finite gradient"""
    m, feat, W = _model("fp32")
    m.create_optimizer()
    p = [W.astype(np.float64), np.array(1.0)]
    mm = [np.zeros_like(p[0]), np.zeros(())]
    vv = [np.zeros_like(p[0]), np.zeros(())]
    step = 0
    for i in range(3):
        b = _batch(32, seed=10 + i)
        m.zero_grad()
        m.forward_backward(b)
        g = [m.param_get("encoder.weight", grad=True).astype(np.float64), m.param_get("logit_scale", grad=True).astype(np.float64)]
        norm, skipped = m.adamw_step(3e-4, 1.0)
        out, rnorm, step = sn.adamw(p, g, mm, vv, step, 3e-4, [0.1, 0.0], 1.0)
        p = [o[0] for o in out]; mm = [o[1] for o in out]; vv = [o[2] for o in out]
        assert not skipped and abs(norm - rnorm) < 1e-4 * rnorm
        assert np.all(m.param_get("encoder.weight", grad=True) == 0)   # the step clears the gradient
    e = _relerr(m.param_get("encoder.weight"), p[0])
    print("adamw relerr", e, m.get_temperature(), float(p[1]))
    assert e < 1e-5
    assert abs(m.get_temperature() - float(p[1])) < 1e-5 * abs(float(p[1]))
    m1, v1, st = m.adamw_state("encoder.weight")
    # the moments: beta2 is an fp32 argument, fl(0.999) = 0.999 + 1.29e-8, so the device's 1 - beta2 is 1e-3 (1 - 1.29e-5) and exp_avg_sq
    # carries that factor whole; rounding a beta to fp32 can cost up to 2^-24 / (1 - beta) = 6e-5, hence 1e-4 (the bias correction
    # divides the factor out again to first order: the parameters above are the tight check)
    assert st == 3 and _relerr(m1, mm[0]) < 1e-4 and _relerr(v1, vv[0]) < 1e-4
    # a non-finite weight makes the gradient non-finite: parameters, moments and the step count stay
    Wd = m.param_get("encoder.weight")
    Wd[3, 7] = np.inf
    m.param_set("encoder.weight", Wd)
    ls1 = m.param_get("logit_scale")
    ms1, vs1, _ = m.adamw_state("logit_scale")
    m.zero_grad()
    m.forward_backward(_batch(32, seed=20))
    norm, skipped = m.adamw_step(3e-4, 1.0)
    assert skipped and not np.isfinite(norm)
    assert m.param_get("encoder.weight").tobytes() == Wd.tobytes()
    assert m.param_get("logit_scale").tobytes() == ls1.tobytes()
    m2, v2, st2 = m.adamw_state("encoder.weight")
    ms2, vs2, _ = m.adamw_state("logit_scale")
    assert st2 == 3
    np.testing.assert_array_equal(m2, m1); np.testing.assert_array_equal(v2, v1)
    np.testing.assert_array_equal(ms2, ms1); np.testing.assert_array_equal(vs2, vs1)
    # the state round trip
    m.adamw_state_set("encoder.weight", m1 * 2, v1 * 3, 7)
    m3, v3, st3 = m.adamw_state("encoder.weight")
    assert st3 == 7
    np.testing.assert_array_equal(m3, m1 * 2); np.testing.assert_array_equal(v3, v1 * 3)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bitwise_reproducible(dtype):
    outs = []
    for _ in range(2):
        m, feat, W = _model(dtype)
        m.create_optimizer()
        losses = []
        for i in range(3):
            m.zero_grad()
            losses.append(m.forward_backward(_batch(37, seed=30 + i))[0])
            m.adamw_step(1e-3, 1.0)
        outs.append((losses, m.param_get("encoder.weight").tobytes(), m.param_get("logit_scale").tobytes()))
        m.close()
    assert outs[0] == outs[1]


def test_export_and_temperature():
    for dtype in ("fp32", "bf16"):   # the export is fp32 arithmetic in both
        m, feat, W = _model(dtype, s=5.0)
        assert _relerr(m.embed(), sn.export(feat, W)) < 1e-5
        assert m.get_temperature() == 5.0


def test_topk_fp32_ties_and_random():
    from recommendersystem_amd import search
    rng = np.random.default_rng(5)
    feat = (rng.standard_normal((V, D)) / np.sqrt(D)).astype(np.float32)
    dup = [5, 700, 2999, 1234]
    for j in dup[1:]:
        feat[j] = feat[dup[0]]            # exact ties: equal rows of E_m give equal scores
    feat[11] = feat[10]
    cfg = search.training_config({0: V}, batch_size=16, embed_dim=D, query_dim=Q)
    m = search.SearchModel(cfg, 0, feat, dtype="fp32")
    W = (rng.standard_normal((Q, D)) * 1.5 / np.sqrt(Q)).astype(np.float32)
    m.param_set("encoder.weight", W)
    x = rng.standard_normal((16, Q)).astype(np.float32)
    pinv = np.linalg.pinv(W.astype(np.float64))            # x Wenc = 8 E_m[5]: the four copies of row 5 lead row 0's list
    x[0] = (8.0 * feat[5].astype(np.float64) @ pinv).astype(np.float32)
    x[1] = (8.0 * feat[10].astype(np.float64) @ pinv).astype(np.float32)
    for k in (1, 4, 50):
        ids, lp = m.topk(x, k)
        rid, rlp = sn.topk(sn.logp(feat, W, 1.0, x), k)
        np.testing.assert_array_equal(ids, rid)
        assert _relerr(lp, rlp) < 1e-4
    ids, _ = m.topk(x[:2], 4)
    assert list(ids[0]) == sorted(dup) and list(ids[1][:2]) == [10, 11]
    ids1, lp1 = m.topk(x[:1], 4)          # a single query takes the column-split path
    np.testing.assert_array_equal(ids1[0], ids[0])


def test_topk_bf16():
    m, feat, W = _model("bf16", max_batch=16)
    x = np.random.default_rng(6).standard_normal((16, Q)).astype(np.float32)
    k = 50
    ids, lp = m.topk(x, k)
    ref = sn.logp(feat, W, 1.0, x, bf16_mode=True)
    tol = 1e-3
    for r in range(16):
        assert len(set(ids[r])) == k
        got = ref[r, ids[r]]
        assert np.all(np.abs(lp[r] - got) <= tol * np.abs(got)), r
        kth = np.sort(ref[r])[-k]
        assert np.all(got >= kth - tol * abs(kth)), r       # near-ties may swap; nothing clearly worse gets in
        assert np.all(np.diff(lp[r]) <= 0)


def test_features_from_model_bitwise():
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import search
    cfg = synth.make_config("hd64", mask_rate=0.2, mask_topk=16)
    cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"] = 3000, 2001
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=4)
    model.init_weights(9)
    model.random_pretrained_embeddings(10)
    Vs = (3000, 2001)
    d = cfg["embed_dim"]
    table = model.item_embeddings()
    rows = {0: table[:Vs[0]], 1: table[Vs[0]:Vs[0] + Vs[1]]}
    rng = np.random.default_rng(2)
    W = (rng.standard_normal((Q, d)) / np.sqrt(Q)).astype(np.float32)
    x = rng.standard_normal((4, Q)).astype(np.float32)
    for medium in (0, 1):
        scfg = search.training_config({0: Vs[0], 1: Vs[1]}, batch_size=8, embed_dim=d, query_dim=Q)
        outs = []
        for features in (model, rows[medium]):
            s = search.SearchModel(scfg, medium, features, dtype="fp32")
            s.param_set("encoder.weight", W)
            outs.append((s.embed().tobytes(), s.topk(x, 8)[1].tobytes()))
            s.close()
        assert outs[0] == outs[1]
    from recommendersystem_amd import RsysError
    with pytest.raises(RsysError):
        search.SearchModel(search.training_config({0: Vs[0] + 1}, batch_size=8, embed_dim=d, query_dim=Q), 0, model, dtype="fp32")


def test_training_lowers_the_test_loss(tmp_path):
    """a planted linear map: queries = E_m[y] A + noise.  Three epochs in fp32 mode; the test loss falls below its epoch -1 value and
    ends no higher than the fp64 restatement's over the same batches, up to the fp32-mode bound"""
    from recommendersystem_amd import search
    v, d, q, bs = 3000, 128, 192, 256
    rng = np.random.default_rng(7)
    feat = (rng.standard_normal((v, d)) / np.sqrt(d)).astype(np.float32)
    A = rng.standard_normal((d, q)) * 3.0

    def chunk(n):
        y = rng.integers(0, v, n)
        return {"queries": (feat[y].astype(np.float64) @ A + 0.3 * rng.standard_normal((n, q))).astype(np.float32), "matchedids": y,
                "mediums": np.where(rng.random(n) < 0.9, 0, 1), "counts": rng.integers(1, 50, n)}

    train_chunks, test_chunks = [chunk(2300), chunk(2300)], [chunk(600)]
    cfg = search.training_config({0: v, 1: 10}, learning_rate=2e-3, batch_size=bs, embed_dim=d, query_dim=q)
    m = search.SearchModel(cfg, 0, feat, dtype="fp32")
    m.init_weights(3)
    W0 = m.param_get("encoder.weight").astype(np.float64)
    mk = lambda: (search.SearchDataset("training", bs, True, 0, chunks=train_chunks, seed=11),
                  search.SearchDataset("test", bs, False, 0, chunks=test_chunks))
    tr, te = mk()
    best = search.train(m, tr, te, str(tmp_path), num_epochs=3, log=lambda s: None)
    rows = open(tmp_path / "search.model.0.csv").read().strip().split("\n")
    assert rows[0] == "epoch,training_loss,test_loss,saved" and rows[1].startswith("-1,inf,") and len(rows) == 5
    test_losses = [float(r.split(",")[2]) for r in rows[1:]]
    assert test_losses[-1] < test_losses[0] and best[1] == min(test_losses)
    ck = search.load_checkpoint(str(tmp_path / "search.model.0.npz"))
    assert ck["encoder.weight"].shape == (q, d) and ck["logit_scale"].shape == ()
    m.load_state_dict(ck)
    out = search.generate_embeddings(m, str(tmp_path))
    with np.load(tmp_path / "output.embeddings.0.npz") as z:
        np.testing.assert_array_equal(z["search.0"], out["search.0"])
        assert z["temperature"][0] == m.get_temperature()
    # the same steps in fp64
    tr, te = mk()
    p = [W0, np.array(1.0)]
    mm = [np.zeros_like(W0), np.zeros(())]; vv = [np.zeros_like(W0), np.zeros(())]
    step = 0

    def ref_eval():
        ls, ws = [], []
        for b in te:
            r = sn.forward_backward(feat, p[0], float(p[1]), b["queries"], b["matchedids"], b["weight"])
            ls.append(r["loss"]); ws.append(r["weight_sum"])
        return sn.epoch_loss(ls, ws)

    ref_losses = [ref_eval()]
    for epoch in range(3):
        for b in tr:
            r = sn.forward_backward(feat, p[0], float(p[1]), b["queries"], b["matchedids"], b["weight"])
            out, _, step = sn.adamw(p, [r["dWenc"], np.array(r["ds"])], mm, vv, step, 2e-3, [0.1, 0.0], 1.0)
            p = [o[0] for o in out]; mm = [o[1] for o in out]; vv = [o[2] for o in out]
        ref_losses.append(ref_eval())
    print("test losses", test_losses, "restatement", ref_losses)
    assert abs(test_losses[0] - ref_losses[0]) < 1e-4 * ref_losses[0]
    assert test_losses[-1] < ref_losses[-1] * (1 + 1e-4)


def test_reference_shaped_step_bf16():
    """one step at train.py's shape (B 1024, D 2048, Q 3072, bf16) with V_m = 80 000: the 256 x 256 score GEMM, two statistics
    workgroups per row, the split-K dP over K = 80 128 summed in split order; the whole batch against the fp64 restatement with
    the device's rounding points (dWenc against x^T dP_ref from that pass), then bitwise reproducibility of the step"""
    v, d, q, B = 80000, 2048, 3072, 1024
    m, feat, W = _model("bf16", 1.0, seed=12, v=v, d=d, q=q, max_batch=B, a=1.5)
    b = _batch(B, seed=13, v=v, q=q)
    outs = []
    for _ in range(2):
        m.zero_grad()
        m.last = m.forward_backward(b)
        outs.append((m.last[0], m.param_get("encoder.weight", grad=True).tobytes(), m.param_get("logit_scale", grad=True).tobytes()))
    assert outs[0] == outs[1]
    ref = sn.forward_backward(feat, W, 1.0, b["queries"], b["matchedids"], b["weight"], bf16_mode=True)
    _check(m, b, ref, 1e-3, "bf16 reference shape")
