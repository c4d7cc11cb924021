"""GPU: the search handle (rsys_search_*, csrc/search.hip) off the shapes of tests/test_gpu_search.py, against tests/_search_np.py: item
counts of 1, a few, and just below / above a multiple of 256 and of 1024 (one statistics split, lanes and waves that see no column, the
padding columns of G), 64 statistics splits with the 32-way ordered split-K dP whose K the splits divide unevenly, a middle split count,
k == V in the top-k call, and an evaluation after a training call.  Every case reads the "splits" debug name back and asserts the path it
names.  Operand scales (_A), tolerances and the comparison (_check) are those of test_gpu_search.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _search_np as sn  # noqa: E402
from test_gpu_search import _A, _batch, _check, _relerr  # noqa: E402

pytestmark = pytest.mark.gpu

D = Q = 64
TOL = {"fp32": 1e-4, "bf16": 1e-3}


def _model(dtype, v, max_batch, s=1.0, a=None, seed=0, dup=None):
    """test_gpu_search._model at D = Q = 64; dup = (i, j): row j of E_m is a copy of row i (an exact tie)"""
    from recommendersystem_amd import search
    rng = np.random.default_rng(seed)
    feat = (rng.standard_normal((v, D)) / np.sqrt(D)).astype(np.float32)
    if dup is not None:
        feat[dup[1]] = feat[dup[0]]
    cfg = search.training_config({0: v}, batch_size=max_batch, embed_dim=D, query_dim=Q)
    m = search.SearchModel(cfg, 0, feat, dtype=dtype, max_batch=max_batch)
    a = _A[dtype][s] if a is None else a
    W = (rng.standard_normal((Q, D)) * a / np.sqrt(Q)).astype(np.float32)
    m.param_set("encoder.weight", W)
    m.param_set("logit_scale", s)
    return m, feat, W


def _splits(m):
    st, k = m.debug("splits", (2,))
    return int(st), int(k)


def _step(m, feat, W, b, dtype, s=1.0, tag=""):
    """one training call from a zero gradient against the restatement; returns the restatement"""
    m.zero_grad()
    m.last = m.forward_backward(b)
    ref = sn.forward_backward(feat, W, s, b["queries"], b["matchedids"], b["weight"], bf16_mode=dtype == "bf16")
    _check(m, b, ref, TOL[dtype], tag)
    return ref


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("v", [5, 255, 257, 1023, 1025])
def test_small_and_off_multiple_v(v, B, dtype):
    """one statistics split (V / 1024 < 2): at V < 1024 lanes, and at V <= 512 whole waves, see no column and hand RowStat{-inf, 0, 0}
    to both sides of stat_merge; Vpad - V padding columns of G (1 at 255 and 1023, 255 at 257 and 1025) enter the K of dP.
    The draws are ones whose loss in the restatement is above 0.05 (asserted): the loss is lse - logit[y], which fp32 resolves to an ulp
    of the logit (1e-6 at 8), so a relative 1e-4 says nothing where the label holds nearly all the mass (a draw at V = 5, B = 1 had a
    loss of 0.0027, at which the restatement evaluated in float32 numpy is itself 9.4e-5 off)"""
    m, feat, W = _model(dtype, v, 4, seed=v)
    ref = _step(m, feat, W, _batch(B, seed=1000 + v + B, v=v, q=Q), dtype, tag=f"{dtype} V={v} B={B}")
    assert ref["loss"] > 0.05
    assert _splits(m) == (1, 1)
    m.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
def test_one_item(B, dtype):
    """V = 1: the soft-max is 1, so lse is the logit, and the loss, dP, dWenc and ds are exactly 0.  With random operands lse is held to
    the restatement at the usual bound; with operands whose products are exact in both modes (x a unit vector, Wenc and E_m multiples of
    1/4, so z is a multiple of 1/16 below 64) the device's logit z expf(1) is within 1 ulp of the restatement's, and lse with it"""
    m, feat, W = _model(dtype, 1, 4, seed=1)
    b = _batch(B, seed=2 + B, v=1, q=Q)
    m.zero_grad()
    loss, wsum = m.forward_backward(b)
    ref = sn.forward_backward(feat, W, 1.0, b["queries"], b["matchedids"], b["weight"], bf16_mode=dtype == "bf16")
    assert _splits(m) == (1, 1)
    assert loss == 0.0 and ref["loss"] == 0.0
    assert _relerr(m.debug("lse", (B,)), ref["lse"]) < TOL[dtype]
    assert not m.debug("dP", (B, D)).any()
    assert not m.param_get("encoder.weight", grad=True).any()
    assert float(m.param_get("logit_scale", grad=True)) == 0.0
    ids, lp = m.topk(b["queries"], 1)
    assert not ids.any() and not lp.any()
    rng = np.random.default_rng(3)
    E1 = rng.integers(-4, 5, (1, D)).astype(np.float32) / 4
    W1 = rng.integers(-4, 5, (Q, D)).astype(np.float32) / 4
    x = np.zeros((B, Q), np.float32)
    x[np.arange(B), rng.integers(0, Q, B)] = 1.0
    from recommendersystem_amd import search
    m1 = search.SearchModel(search.training_config({0: 1}, batch_size=4, embed_dim=D, query_dim=Q), 0, E1, dtype=dtype, max_batch=4)
    m1.param_set("encoder.weight", W1)
    m1.param_set("logit_scale", 1.0)
    b1 = {"queries": x, "matchedids": np.zeros(B, np.int64), "weight": np.ones(B)}
    m1.zero_grad()
    loss1, _ = m1.forward_backward(b1)
    ref1 = sn.forward_backward(E1, W1, 1.0, x, b1["matchedids"], b1["weight"], bf16_mode=dtype == "bf16")
    want = ref1["lse"].astype(np.float32)
    got = m1.debug("lse", (B,))
    ulps = np.abs(got.astype(np.float64) - ref1["lse"]) / np.spacing(np.abs(want)).astype(np.float64)
    print("V=1 exact operands: lse", got, "restatement", ref1["lse"], "ulps", ulps)
    assert loss1 == 0.0 and np.all(ulps <= 1.0)
    m.close()
    m1.close()


def _no_near_tie(ref_row, dup, gap):
    """the restatement's sorted log-probabilities of a row are at least `gap` apart, the planted duplicate aside"""
    o = np.argsort(-ref_row, kind="stable")
    d = -np.diff(ref_row[o])
    planted = np.array([{int(o[i]), int(o[i + 1])} == set(dup) for i in range(len(o) - 1)]) if dup else np.zeros(len(d), bool)
    return bool(np.all(d[~planted] > gap)) and (not dup or bool(np.all(d[planted] == 0)))


@pytest.mark.parametrize("v", [5, 257])
def test_topk_all_items_fp32(v):
    """k == V: every item is returned, in the restatement's stable order; rows 2 and 3 of E_m are equal, so every query has an exact tie
    that the ascending id decides.  The draw is one whose other neighbours are at least 1e-4 apart in the restatement (asserted): the
    worst-case fp32 error of a logit here is 2 K u sum |P_k E_k| exp(s) ~ 2e-5 (K = 64, u = 6e-8, |P| |E| ~ 1.5), so no other pair can
    swap"""
    dup = (2, 3)
    m, feat, W = _model("fp32", v, 4, seed=42 + v, dup=dup)
    x = np.random.default_rng(43 + v).standard_normal((3, Q)).astype(np.float32)
    ref = sn.logp(feat, W, 1.0, x)
    assert all(_no_near_tie(r, dup, 1e-4) for r in ref)
    for nq in (1, 3):
        ids, lp = m.topk(x[:nq], v)
        rid, rlp = sn.topk(ref[:nq], v)
        np.testing.assert_array_equal(ids, rid)
        assert _relerr(lp, rlp) < 1e-4
        assert all(list(r).index(2) + 1 == list(r).index(3) for r in ids)
    assert _splits(m) == (1, 0)
    m.close()


@pytest.mark.parametrize("v", [5, 257])
def test_topk_all_items_bf16(v):
    """k == V under test_topk_bf16's near-tie rule: a permutation of all ids, every value the restatement's for its id, descending"""
    m, feat, W = _model("bf16", v, 4, seed=50 + v)
    x = np.random.default_rng(51 + v).standard_normal((3, Q)).astype(np.float32)
    ids, lp = m.topk(x, v)
    ref = sn.logp(feat, W, 1.0, x, bf16_mode=True)
    tol = 1e-3
    for r in range(3):
        assert sorted(ids[r]) == list(range(v))
        got = ref[r, ids[r]]
        assert np.all(np.abs(lp[r] - got) <= tol * np.abs(got)), r
        kth = np.sort(ref[r])[-v]
        assert np.all(got >= kth - tol * abs(kth)), r
        assert np.all(np.diff(lp[r]) <= 0)
    m.close()


@pytest.fixture(scope="module")
def big():
    """V = 70001, B = 3: min(64, ceil(2048 / 3), 70001 / 1024) = 64 statistics splits of 1096 columns; Vpad = 70144, and dP asks for
    min(64, 70144 / 2048, 2048 / 2 tiles) = 34 -> 32 ordered K splits of 2192 rows, not a whole number of K tiles.  One handle per dtype,
    made on first use."""
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = _model(dtype, 70001, 4, seed=70)
        return made[dtype]
    yield get
    for m, _, _ in made.values():
        m.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_64_statistics_splits(big, dtype):
    m, feat, W = big(dtype)
    m.param_set("encoder.weight", W)
    m.param_set("logit_scale", 1.0)
    b = _batch(3, seed=71, v=70001, q=Q)
    _step(m, feat, W, b, dtype, tag=f"{dtype} V=70001 B=3")
    st, ks = _splits(m)
    assert st == 64 and ks == 32
    first = (m.last[0], m.debug("lse", (3,)).tobytes(), m.debug("dP", (3, D)).tobytes(), m.param_get("encoder.weight", grad=True).tobytes(),
             m.param_get("logit_scale", grad=True).tobytes())
    m.zero_grad()
    again = m.forward_backward(b)
    assert first == (again[0], m.debug("lse", (3,)).tobytes(), m.debug("dP", (3, D)).tobytes(),
                     m.param_get("encoder.weight", grad=True).tobytes(), m.param_get("logit_scale", grad=True).tobytes())


def test_64_statistics_splits_large_logits_fp32(big):
    """s = 5 with a = 0.2: logits of std 30, so the 64-way merge rescales partial sums across splits whose maxima differ by more than
    log(FLT_MAX)"""
    m, feat, _ = big("fp32")
    W = (np.random.default_rng(72).standard_normal((Q, D)) * _A["fp32"][5.0] / np.sqrt(Q)).astype(np.float32)
    m.param_set("encoder.weight", W)
    m.param_set("logit_scale", 5.0)
    ref = _step(m, feat, W, _batch(3, seed=73, v=70001, q=Q), "fp32", s=5.0, tag="fp32 V=70001 B=3 s=5")
    assert ref["z"].max() > 88.8
    st, ks = _splits(m)
    assert st == 64 and ks > 1


def test_middle_split_count_fp32():
    """V = 9001, B = 300: min(64, ceil(2048 / 300), 9001 / 1024) = 7 statistics splits of 1288 columns, the last one short"""
    m, feat, W = _model("fp32", 9001, 300, seed=90)
    _step(m, feat, W, _batch(300, seed=91, v=9001, q=Q), "fp32", tag="fp32 V=9001 B=300")
    assert _splits(m)[0] == 7
    m.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_evaluate_after_train(dtype):
    v = 257
    m, feat, W = _model(dtype, v, 4, seed=60)
    _step(m, feat, W, _batch(3, seed=61, v=v, q=Q), dtype, tag=f"{dtype} V=257 train")
    g, gs = m.param_get("encoder.weight", grad=True), m.param_get("logit_scale", grad=True)
    assert g.any()
    b = _batch(2, seed=62, v=v, q=Q)
    loss, _ = m.forward_backward(b, evaluate=True)
    ref = sn.forward_backward(feat, W, 1.0, b["queries"], b["matchedids"], b["weight"], bf16_mode=dtype == "bf16")
    assert abs(loss - ref["loss"]) < TOL[dtype] * ref["loss"]
    assert _relerr(m.debug("lse", (2,)), ref["lse"]) < TOL[dtype]
    assert m.param_get("encoder.weight", grad=True).tobytes() == g.tobytes()
    assert m.param_get("logit_scale", grad=True).tobytes() == gs.tobytes()
    assert _splits(m) == (1, 0)
    m.close()
