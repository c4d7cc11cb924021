"""GPU: the item-similarity handle (rsys_sim_*, csrc/similarity.hip) off the power-of-two shapes of tests/test_gpu_similarity.py, against
tests/_similarity_np.py (whose gradients tests/test_similarity_host.py holds to autograd): list lengths that the rank sort pads, that leave
the last pair-loss workgroup and the last pair workgroup part empty, n = 1; the evaluation row map; a list without pairs; a small call after
a large one on one handle; ordered split-K weight gradients at split counts the caller did not round; the clamp branch of the normalisation
backward; nDCG and the hard-negative fill at small V.

Every parity case first asserts ranks == sn.ranks(device scores) exactly and then feeds the device's ranks to the restatement, so no near-tie
can flip a rank between the two.  Tolerances are those of test_gpu_similarity.py: 1e-4 in fp32 and 1e-3 in bf16 for loss, dldx, dW and dls,
1e-5 / 1e-2 for the scores."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _similarity_np as sn  # noqa: E402
from test_gpu_similarity import _check_grads, _relerr  # noqa: E402

pytestmark = pytest.mark.gpu

V, F, E, MAXQ, NMAX = 3000, 64, 64, 16, 2048
TOL = {"fp32": 1e-4, "bf16": 1e-3}
TOL_X = {"fp32": 1e-5, "bf16": 1e-2}
SHAPES = [(1, 1), (3, 2), (5, 3), (7, 63), (7, 65), (3, 255), (9, 300), (2, 1025), (1, 2047)]


def _handle(dtype, dropout=0.0, v=V, nmax=NMAX, maxq=MAXQ, seed=0, feat=None, W=None):
    from recommendersystem_amd import similarity as sim
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((v, F)).astype(np.float32) if feat is None else feat
    W = (rng.standard_normal((E, F)) / np.sqrt(F)).astype(np.float32) if W is None else W
    m = sim.LTRModel(sim.training_config({0: v}, embed_dim=E, batch_size=maxq, items_per_query=nmax), 0, feat, dtype=dtype, dropout=dropout)
    m.param_set("encoder.1.weight", W)
    return m, feat, W


@pytest.fixture(scope="module")
def handles():
    """one fp32 and one bf16 handle for the module (V 3000, F 64, E 64, 16 queries of up to 2048 items, no dropout), made on first use"""
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = _handle(dtype)
        return made[dtype]
    yield get
    for m, _, _ in made.values():
        m.close()


def _lists(nq, n, seed, v=V):
    """targets without replacement; every list has at least two distinct relevances (n > 1) and repeated ones"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, v, nq)
    tgt = np.stack([rng.permutation(v)[:n] for _ in range(nq)])
    rel = np.where(rng.random((nq, n)) < 0.3, rng.integers(1, 6, (nq, n)).astype(np.float64), 0.0)
    if n > 1:
        rel[:, 0], rel[:, 1] = 3.0, 0.0
    w = np.sqrt(rng.integers(1, 100, nq).astype(np.float64))
    return {"sourceid": np.repeat(src[:, None], n, 1), "targetid": tgt, "relevance": rel, "weight": w[:, None]}


_REF = {}


def _reference(feat, W, ls, b, order, dtype, key):
    """sn.forward_backward_by_id fed the device's ranks; computed once per (case, dtype, ranks) and shared by the tests of that case"""
    key = (key, dtype, order.tobytes())
    if key not in _REF:
        _REF[key] = sn.forward_backward_by_id(feat, W, ls, b["sourceid"][:, 0], b["targetid"], b["relevance"], b["weight"][:, 0], order,
                                              bf16_mode=dtype == "bf16")
    return _REF[key]


def _ranks_and_scores(m, nq, n):
    """the device's ranks, asserted to be the stable descending order of the device's own scores"""
    x = m.debug("scores", (nq, n), np.float32)
    order = m.debug("ranks", (nq, n), np.int32)
    np.testing.assert_array_equal(order, sn.ranks(x))
    return order, x


def _grads(m):
    return m.param_get("encoder.1.weight", grad=True), m.param_get("logit_scale", grad=True)


def _ksplits(m):
    return int(m.debug("splits", (1,), np.int32)[0])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("nq,n", SHAPES)
def test_ragged_lists_training(handles, nq, n, dtype):
    """n that the rank sort pads to the next power of two (3, 63, 65, 255, 300, 1025, 2047), n = 1 (no sort step) and 2; n_q n pairs that
    leave the last pair workgroup of 4 with 1 (1, 441, 765), 2 (6, 2050) or 3 (15, 455, 2047) live pairs; last pair-loss workgroups of
    256 with 1 (n = 1025), 44 (300), 63, 65 or 255 (255, 2047) live slots, alone or behind full ones"""
    m, feat, W = handles(dtype)
    b = _lists(nq, n, seed=100 * nq + n)
    m.zero_grad()
    loss = m.forward_backward(b)
    order, x = _ranks_and_scores(m, nq, n)
    ref_loss, rx, g, dW, dls = _reference(feat, W, m.get_temperature(), b, order, dtype, (nq, n))
    assert _relerr(x, rx) < TOL_X[dtype]
    if n == 1:   # no pair: exact zeros, no ratio
        assert loss == 0.0 and ref_loss == 0.0 and dls == 0.0
        assert not m.debug("dldx", (nq, n), np.float32).any()
        gW, gls = _grads(m)
        assert not gW.any() and float(gls) == 0.0
        return
    _check_grads(m, loss, ref_loss, g, dW, dls, nq, n, tol_loss=TOL[dtype], tol=TOL[dtype])
    assert _ksplits(m) >= 1


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("nq,n", SHAPES)
def test_ragged_lists_evaluation(handles, nq, n, dtype):
    """evaluate=True: one source row per query (row pair / n of Y), n_q + n_q n gathered rows; loss and scores against the restatement,
    the gradients bit for bit what the training call before it left"""
    m, feat, W = handles(dtype)
    m.zero_grad()
    m.forward_backward(_lists(4, 37, seed=7))
    gW, gls = _grads(m)
    assert gW.any()
    b = _lists(nq, n, seed=100 * nq + n)
    loss = m.forward_backward(b, evaluate=True)
    order, x = _ranks_and_scores(m, nq, n)
    ref_loss, rx, _, _, _ = _reference(feat, W, m.get_temperature(), b, order, dtype, (nq, n))
    assert _relerr(x, rx) < TOL_X[dtype]
    xe = sn.scores_eval(feat, W, m.get_temperature(), b["sourceid"][:, 0], b["targetid"], bf16_mode=dtype == "bf16")
    assert _relerr(x, xe) < TOL_X[dtype]
    if n == 1:
        assert loss == 0.0 and ref_loss == 0.0
    else:
        assert abs(loss - ref_loss) / abs(ref_loss) < TOL[dtype], (loss, ref_loss)
    gW2, gls2 = _grads(m)
    assert gW2.tobytes() == gW.tobytes() and gls2.tobytes() == gls.tobytes()
    assert _ksplits(m) == 0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_a_list_without_pairs(handles, dtype):
    m, feat, W = handles(dtype)
    nq, n = 4, 65
    b = _lists(nq, n, seed=21)
    b["relevance"][2] = 2.0
    m.zero_grad()
    loss = m.forward_backward(b)
    order, x = _ranks_and_scores(m, nq, n)
    ref_loss, rx, g, dW, dls = _reference(feat, W, m.get_temperature(), b, order, dtype, "no pairs")
    d = m.debug("dldx", (nq, n), np.float32)
    assert not d[2].any() and not g[2].any()
    assert d[[0, 1, 3]].any(axis=1).all()
    _check_grads(m, loss, ref_loss, g, dW, dls, nq, n, tol_loss=TOL[dtype], tol=TOL[dtype])


def _one_step(m, b, check_ranks=True, **kw):
    m.zero_grad()
    loss = m.forward_backward(b, **kw)
    nq, n = b["targetid"].shape
    if check_ranks:
        _ranks_and_scores(m, nq, n)
    gW, gls = _grads(m)
    return loss, m.debug("dldx", (nq, n), np.float32).tobytes(), gW.tobytes(), gls.tobytes()


@pytest.mark.parametrize("dropout", [0.0, 0.1])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_small_after_large(dtype, dropout):
    """(9, 300) and then (3, 2) on one handle: rows [12, 256) of X, Y and dY hold the larger call's values unless the small call clears
    them, and the K-major dW product runs over all 256; every output of the second call is bitwise that of a fresh handle.  (Finite
    leftovers in dY alone meet the zero rows of X and add exact zeros: the next test is the one that sees dY left uncleared.)"""
    kw = {"seed": 5, "step": 9} if dropout else {}
    big, small = _lists(9, 300, seed=31), _lists(3, 2, seed=32)
    a, _, _ = _handle(dtype, dropout, nmax=300)
    _one_step(a, big, **kw)
    got = _one_step(a, small, **kw)
    f, _, _ = _handle(dtype, dropout, nmax=300)
    want = _one_step(f, small, **kw)
    assert got == want
    assert np.frombuffer(want[2], np.float32).any()
    a.close()
    f.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_small_after_a_non_finite_large_call(dtype):
    """the same after a call whose source row held inf (the step an AdamW skip follows): that call leaves NaN in rows of dY that the
    small call does not write, and 0 x NaN is not 0; with the features restored the small call is bitwise that of a fresh handle"""
    from recommendersystem_amd._lib import check, lib
    big, small = _lists(9, 300, seed=31), _lists(3, 2, seed=32)
    a, feat, _ = _handle(dtype, nmax=300)
    bad = feat.copy()
    bad[big["sourceid"][0, 0]] = np.inf
    check(lib().rsys_sim_features_set(a.h, bad.ctypes.data_as(C.c_void_p), V, F))
    _one_step(a, big, check_ranks=False)
    assert not np.isfinite(_grads(a)[0]).all()
    check(lib().rsys_sim_features_set(a.h, feat.ctypes.data_as(C.c_void_p), V, F))
    got = _one_step(a, small)
    f, _, _ = _handle(dtype, nmax=300)
    want = _one_step(f, small)
    assert got == want
    assert np.isfinite(np.frombuffer(got[2], np.float32)).all()
    a.close()
    f.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("nq,n", [(9, 500), (11, 2047)])
def test_uneven_ordered_split_k(handles, nq, n, dtype):
    """(9, 500): R = 9000, Rpad = 9216, 2 K splits requested; (11, 2047): Rpad = 45056, 11 requested.  The route rounds either count, the
    partial tiles are summed in split order: dW against the restatement, more than one split read back, and a repeated call bitwise equal"""
    m, feat, W = handles(dtype)
    b = _lists(nq, n, seed=100 * nq + n)
    first = _one_step(m, b)
    assert _ksplits(m) > 1
    order, x = _ranks_and_scores(m, nq, n)
    ref_loss, rx, g, dW, dls = _reference(feat, W, m.get_temperature(), b, order, dtype, (nq, n))
    _check_grads(m, first[0], ref_loss, g, dW, dls, nq, n, tol_loss=TOL[dtype], tol=TOL[dtype])
    assert _one_step(m, b) == first


def test_dropout_at_a_ragged_shape_fp32():
    p, nq, n = 0.1, 7, 65
    m, feat, W = _handle("fp32", p, nmax=65)
    b = _lists(nq, n, seed=41)
    m.zero_grad()
    loss = m.forward_backward(b, seed=7, step=3)
    mask = m.debug("dropout_mask", (2 * nq * n, F), np.uint8).astype(bool)
    assert 0.85 < mask.mean() < 0.95
    ms, mt = mask[:nq * n], mask[nq * n:]
    assert not np.array_equal(ms[0], ms[1])
    ref_loss, x, g, dW, dls = sn.forward_backward(feat, W, m.get_temperature(), b["sourceid"][:, 0], b["targetid"], b["relevance"],
                                                  b["weight"][:, 0], masks=(ms, mt), p=p)
    np.testing.assert_array_equal(m.debug("ranks", (nq, n), np.int32), sn.ranks(m.debug("scores", (nq, n), np.float32)))
    assert abs(loss - ref_loss) / abs(ref_loss) < 1e-4
    assert _relerr(m.param_get("encoder.1.weight", grad=True), dW) < 1e-4
    m.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_clamp_branch(dtype):
    """a target whose feature row is e_0 under a W whose column 0 is zero: its Y row is exactly zero, |Y| <= 1e-12 takes the clamp branch
    (dY = gd a / 1e-12), its score is +0.0, and since its X row is e_0 the whole of that dY lands in column 0 of dW, ~1e12 dL/dx; the other
    columns get nothing from it.  Column 0 and the rest are compared separately, so neither hides the other"""
    nq, n = 3, 5
    rng = np.random.default_rng(51)
    feat = rng.standard_normal((V, F)).astype(np.float32)
    W = (rng.standard_normal((E, F)) / np.sqrt(F)).astype(np.float32)
    b = _lists(nq, n, seed=52)
    zid = int(np.setdiff1d(np.arange(V), np.concatenate([b["sourceid"][:, 0], b["targetid"].reshape(-1)]))[0])
    b["targetid"][1, 2] = zid
    b["relevance"][1] = [0.0, 2.0, 4.0, 0.0, 1.0]
    feat[zid] = 0.0
    feat[zid, 0] = 1.0
    W[:, 0] = 0.0
    m, _, _ = _handle(dtype, nmax=8, maxq=4, feat=feat, W=W)
    m.zero_grad()
    loss = m.forward_backward(b)
    order, x = _ranks_and_scores(m, nq, n)
    assert x[1, 2] == 0.0 and not np.signbit(x[1, 2])
    ref_loss, rx, g, dW, dls = _reference(feat, W, m.get_temperature(), b, order, dtype, "clamp")
    assert rx[1, 2] == 0.0 and abs(g[1, 2]) > 0 and np.abs(dW[:, 0]).max() > 1e10 * abs(g[1, 2])
    tol = TOL[dtype]
    assert abs(loss - ref_loss) / abs(ref_loss) < tol
    assert _relerr(m.debug("dldx", (nq, n), np.float32), g) < tol
    gW, gls = _grads(m)
    e0, er = _relerr(gW[:, 0], dW[:, 0]), _relerr(gW[:, 1:], dW[:, 1:])
    print("clamp", dtype, "dW column 0", e0, "other columns", er)
    assert e0 < tol and er < tol
    assert abs(float(gls) - dls) <= tol * max(abs(dls), 1e-3)
    m.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 3, 257, 2047])
def test_ndcg_ragged_with_ties(handles, n, dtype):
    """odd slots repeat the even slots' targets, so half the scores tie; sn.ndcg on the device's scores, as test_ndcg_with_ties"""
    m, feat, W = handles(dtype)
    nq = 5
    b = _lists(nq, n, seed=60 + n)
    b["targetid"][:, 1::2] = b["targetid"][:, 0:n - 1:2]
    b["relevance"][:, 0] = 3.0
    s, w = m.ndcg(b)
    _, x = _ranks_and_scores(m, nq, n)
    if n > 1:
        assert np.any(x[:, 0:n - 1:2] == x[:, 1::2])
    rs, rw = sn.ndcg(x, b["relevance"], b["weight"][:, 0].astype(np.float32))
    assert abs(w - rw) < 1e-9 * rw
    assert abs(s - rs) < 1e-5 * rw
    xr = sn.scores_eval(feat, W, m.get_temperature(), b["sourceid"][:, 0], b["targetid"], bf16_mode=dtype == "bf16")
    assert _relerr(x, xr) < TOL_X[dtype]
    # one list without a relevant item: DCG 0 over IDCG 0, as the reference divides
    b["relevance"][nq // 2] = 0.0
    s, w = m.ndcg(b)
    with np.errstate(invalid="ignore", divide="ignore"):
        rs, _ = sn.ndcg(x, b["relevance"], b["weight"][:, 0].astype(np.float32))
    assert np.isnan(rs) and np.isnan(s) and abs(w - rw) < 1e-9 * rw


def _hard_negative_case(v, n, sources, positives, tm, seed):
    """integer embeddings: every dot product is exact in fp32, the bf16-rounded scores are known exactly and tie a lot"""
    rng = np.random.default_rng(seed)
    m, _, _ = _handle("fp32", v=v, nmax=n, maxq=2)
    emb = rng.integers(-3, 4, (v, E)).astype(np.float32)
    emb[3:6] = emb[2]
    m.set_export(emb)
    m.set_testmask(tm)
    sc = sn.bf16(emb.astype(np.float64) @ emb.astype(np.float64).T)
    fills = {}
    for split in ("training", "test"):
        out = m.hard_negatives(split, sources, positives, n)
        for i, s in enumerate(sources):
            ref = sn.hard_negatives(sc[s], s, tm[s], split, positives[i], n)
            np.testing.assert_array_equal(out[i], ref, err_msg=f"{split} source {s}")
            w = np.ones(v, bool)
            w[s] = False
            w[tm[s] if split == "training" else ~tm[s]] = False
            w[positives[i]] = False
            fills[(split, i)] = n - min(n, int(w.sum()))
    m.close()
    return fills


def test_hard_negatives_every_item():
    """V = 37, n = V: a source is never its own negative, so every row has a fill; one 256-column step that is mostly beyond V"""
    v = 37
    rng = np.random.default_rng(70)
    tm = rng.random((v, v)) < 0.4
    sources = list(range(v))
    positives = [rng.integers(0, v, k).tolist() for k in rng.integers(0, 6, v)]
    fills = _hard_negative_case(v, v, sources, positives, tm, 71)
    assert min(fills.values()) >= 1


def test_hard_negatives_v_257():
    """V = 257 (one column into a second 256-column step), n = 200"""
    v, n = 257, 200
    rng = np.random.default_rng(72)
    tm = rng.random((v, v)) < 0.5
    tm[7] = True
    tm[8] = False
    sources = [0, 7, 8, 2, 4, 255, 256] + rng.integers(0, v, 20).tolist()
    positives = [rng.integers(0, v, k).tolist() for k in rng.integers(0, 30, len(sources))]
    fills = _hard_negative_case(v, n, sources, positives, tm, 73)
    assert max(fills.values()) == n and min(fills.values()) == 0


def test_hard_negatives_long_fill():
    """V = 700, n = 600: sources whose mask row and positives leave fewer than 50 admissible ids, so more than 256 ids are filled and the
    walk over the inadmissible ids takes a second and a third 256-column step; sources with no admissible id at all"""
    v, n = 700, 600
    rng = np.random.default_rng(74)
    tm = rng.random((v, v)) < 0.5
    few_test, few_train, none_test, none_train = [11, 300], [12, 699], 13, 14
    for s in few_test:       # the test split admits the set bits
        tm[s] = False
        tm[s, rng.permutation(v)[:45]] = True
    for s in few_train:      # the training split admits the clear bits
        tm[s] = True
        tm[s, rng.permutation(v)[:45]] = False
    tm[none_test] = False
    tm[none_train] = True
    sources = few_test + few_train + [none_test, none_train] + rng.integers(0, v, 14).tolist()
    positives = [rng.integers(0, v, k).tolist() for k in rng.integers(0, 40, len(sources))]
    fills = _hard_negative_case(v, n, sources, positives, tm, 75)
    assert all(fills[("test", i)] > 512 for i in (0, 1)) and all(fills[("training", i)] > 512 for i in (2, 3))
    assert fills[("test", 4)] == n and fills[("training", 5)] == n
