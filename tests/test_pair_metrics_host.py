"""CPU: the host side of the catalogue metrics (similarity.py dcg_at_k, ndcg_at_k, recall_at_k, make_metric_dataframe, metric_frame)
against tests/_pairwise_metrics_np.py, a restatement of pairwise_metrics.jl read from its source (Julia is not available, so the
restatement is not pinned against Julia's output).  The host functions take ranks where the reference sorts; fed the restatement's own
ranks they must reproduce its six numbers to 1e-12 relative (the same fp64 operations; the summation order may differ by a few terms)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pairwise_metrics_np as pm  # noqa: E402

from recommendersystem_amd import similarity as sim  # noqa: E402

RTOL = 1e-12


def _ranks(df, M):
    return np.array([pm.ranks_of(M[s], s, [t])[0] for s, t in zip(df["source"], df["target"])], np.int32)


def _six(df, M, ks=pm.KS):
    ranks = _ranks(df, M)
    got, ref = {}, {}
    for k in ks:
        got[f"nDCG@{k}"] = sim.ndcg_at_k(df, ranks, k); ref[f"nDCG@{k}"] = pm.ndcg_at_k(df, M, k)
        got[f"Recall@{k}"] = sim.recall_at_k(df, ranks, k); ref[f"Recall@{k}"] = pm.recall_at_k(df, M, k)
    return got, ref


def _close(got, ref):
    for name in ref:
        assert abs(got[name] - ref[name]) <= RTOL * abs(ref[name]), (name, got[name], ref[name])


def test_isless_order_of_the_restatement():
    x = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-30, -1e-30, -np.nan, 1.0, 0.0], np.float32)
    order = pm.sortperm_rev(x)
    # NaNs first (equal: by position), +inf, 1, 1e-30, +0.0 (twice, by position), -0.0, -1e-30, -inf
    np.testing.assert_array_equal(order, [2, 7, 3, 8, 5, 0, 9, 1, 6, 4])
    np.testing.assert_array_equal(pm.ranks_of(x, 3, [2, 7, 3, 9, 4]), [1, 2, 0, 6, 9])


def test_dcg_at_k():
    rel = [3.0, 0.0, 1.5, 2.0]
    for k in (0, 1, 3, 10):
        assert sim.dcg_at_k(rel, k) == pm.dcg_at_k(rel, k)
    assert sim.dcg_at_k([], 8) == 0.0


def test_frame_filters_rows_as_save_metrics():
    emb, tm, pairs = pm.toy_catalogue(60, 16, 3, 20, medium=1)
    got, ref = sim.metric_frame(pairs, tm, 1), pm.metric_frame(pairs, tm, 1)
    assert len(ref["source"]) > 40 and len(ref["source"]) < len(pairs["score"])
    for k in ref:
        np.testing.assert_array_equal(np.asarray(got[k]), np.asarray(ref[k]))
    assert len(sim.metric_frame(pairs, tm, 0)["source"]) == 0   # cliptype "medium1" only


def test_metrics_match_the_restatement():
    """duplicated targets (the last relevance wins in the dict, every row counts in the recall's denominator), repeated (source,
    popularity) groups (the first row's weight), targets beyond k, and k > V - 1"""
    emb, tm, pairs = pm.toy_catalogue(300, 32, 5, 80, medium=0, density=0.3, max_targets=12)
    df = pm.metric_frame(pairs, tm, 0)
    M = pm.masked_gram(emb, tm)
    ranks = _ranks(df, M)
    assert ranks.min() >= 1 and (ranks > 8).any() and (ranks > 128).any() and ranks.max() <= 299
    pairs_seen = list(zip(df["source"], df["target"]))
    assert len(set(pairs_seen)) < len(pairs_seen)                               # duplicated targets
    assert len({(s, w) for s, w in zip(df["source"], df["weight"])}) > len(set(df["source"]))   # a source with two popularities
    got, ref = _six(df, M)                                                       # k = 1024 > V - 1 = 299
    _close(got, ref)
    assert 0 < ref["nDCG@8"] < ref["nDCG@1024"] <= 1 and 0 < ref["Recall@8"] < 1
    assert got["nDCG@1024"] == sim.ndcg_at_k(df, ranks, 299)


def test_zero_score_rows_do_not_reach_the_metrics():
    """a source whose only rows have score 0 is dropped by the frame's filter, so no recall divides by a zero relevance sum"""
    emb, tm, pairs = pm.toy_catalogue(80, 16, 9, 10, medium=0)
    s = next(i for i in range(1, 80) if i not in set(pairs["source_matchedid"]) and tm[i].any())
    t = int(np.flatnonzero(tm[s])[0])
    for k, v in (("cliptype", "medium0"), ("source_matchedid", s), ("source_popularity", 5.0), ("target_matchedid", t), ("score", 0.0)):
        pairs[k] = np.append(pairs[k], v)
    df = sim.metric_frame(pairs, tm, 0)
    assert s not in set(df["source"].tolist())
    M = pm.masked_gram(emb, tm)
    got, ref = _six(pm.metric_frame(pairs, tm, 0), M)
    _close(got, ref)
    assert all(np.isfinite(v) for v in got.values())


def test_target_equal_to_its_source_counts_in_the_ideal_only():
    """a (source, source) row is in the dict (IDCG, recall denominator) but is no candidate: rank 0"""
    V = 40
    emb, tm, _ = pm.toy_catalogue(V, 16, 11, 5, medium=0)
    tm[7, 7] = True
    df = {"source": [7, 7, 7], "target": [7, 3, 9], "relevance": [2.0, 1.0, 0.5], "weight": [2.0, 2.0, 2.0]}
    M = pm.masked_gram(emb, tm)
    ranks = _ranks(df, M)
    assert ranks[0] == 0 and ranks[1] >= 1
    got, ref = _six(df, M, ks=(1, 8, 1024))
    _close(got, ref)


def test_metric_frame_columns():
    d = {f"{m}.{name}@{k}": float(m + k) for m in (1, 0) for name in ("nDCG", "Recall") for k in (1024, 8, 128)}
    cols, rows = sim.make_metric_dataframe(d)
    assert cols == ["medium", "Recall@8", "Recall@128", "Recall@1024", "nDCG@8", "nDCG@128", "nDCG@1024"]
    assert rows == [[0, 8.0, 128.0, 1024.0, 8.0, 128.0, 1024.0], [1, 9.0, 129.0, 1025.0, 9.0, 129.0, 1025.0]]
