"""numpy restatement of Training/item_similarity/pairwise_metrics.jl (save_metrics, ndcg_at_k, recall_at_k, dcg_at_k), read from its
source.  Julia is not available where the tests run, so this is a RESTATEMENT of the file's arithmetic, not a pin against its output:
the dense `M = E' * E` in Float32 times the Int8 test mask, per source a stable sort of all other items under `isless` with rev = true,
the `Dict(target => relevance)` (a repeated target keeps its last relevance) and the loops as the file writes them.  Ids are 0-based."""
import math

import numpy as np

KS = (8, 128, 1024)


def isless_key(x):
    """uint32 keys ordered as Julia's isless on Float32: -inf < ... < -0.0 < +0.0 < ... < +inf < NaN (all NaNs equal)"""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(x)] = np.uint32(0xFFFFFFFF)
    return k


def sortperm_rev(x):
    """sortperm(x, rev = true): descending under isless, equal values in their original order (the sort is stable)"""
    return np.argsort(np.int64(0xFFFFFFFF) - isless_key(x).astype(np.int64), kind="stable")


def masked_gram(E, testmask):
    """M = E' * E in Float32, then M .* testmask (an IEEE product with 0 or 1: a masked zero keeps the sign, inf * 0 is NaN)"""
    E = np.asarray(E, np.float32)
    with np.errstate(invalid="ignore"):
        return (E @ E.T).astype(np.float32) * np.asarray(testmask).astype(np.float32)


def ranked_items(row, source_id):
    """candidate_items[sortperm(predictions[candidate_items], rev = true)] (pairwise_metrics.jl:85-87)"""
    candidates = np.array([i for i in range(len(row)) if i != source_id], np.int64)
    return candidates[sortperm_rev(np.asarray(row, np.float32)[candidates])]


def ranks_of(row, source_id, targets):
    """1-based position of each target in ranked_items, 0 for the source itself"""
    pos = {int(item): r + 1 for r, item in enumerate(ranked_items(row, source_id))}
    return np.array([pos.get(int(t), 0) for t in targets], np.int32)


def dcg_at_k(relevances, k):
    n = min(k, len(relevances))
    score = 0.0
    for i in range(1, n + 1):
        score += relevances[i - 1] / math.log2(i + 1)
    return score


def _groups(df):
    """unique(df.source) and groupby(df, :source; sort = false): row indices per source, sources in order of first appearance"""
    groups = {}
    for i, s in enumerate(df["source"]):
        groups.setdefault(int(s), []).append(i)
    return groups


def ndcg_at_k(df, M, k):
    weighted, weights = [], []
    for source_id, rows in _groups(df).items():
        weight = df["weight"][rows[0]]
        true_relevances = {int(df["target"][i]): float(df["relevance"][i]) for i in rows}
        items = ranked_items(M[source_id], source_id)
        ranked_relevances = [true_relevances.get(int(item), 0.0) for item in items]
        dcg = dcg_at_k(ranked_relevances, k)
        ideal = sorted(true_relevances.values(), reverse=True)
        idcg = dcg_at_k(ideal, k)
        ndcg = dcg / idcg if idcg > 0 else 0.0
        weighted.append(ndcg * weight)
        weights.append(weight)
    return sum(weighted) / sum(weights)


def recall_at_k(df, M, k):
    weighted, weights = [], []
    for source_id, rows in _groups(df).items():
        items = ranked_items(M[source_id], source_id)
        top_k_items = items[:min(k, len(items))]
        counts = {int(df["target"][i]): float(df["relevance"][i]) for i in rows}
        count_in_top_k = sum(counts.get(int(item), 0) for item in top_k_items)
        recall = count_in_top_k / sum(float(df["relevance"][i]) for i in rows)
        weight = df["weight"][rows[0]]
        weighted.append(recall * weight)
        weights.append(weight)
    return sum(weighted) / sum(weights)


def metric_frame(pairs, testmask, medium):
    """save_metrics, :164-172"""
    keep = [i for i in range(len(pairs["score"]))
            if str(pairs["cliptype"][i]) == f"medium{medium}" and pairs["score"][i] != 0]
    keep = [i for i in keep if testmask[pairs["source_matchedid"][i], pairs["target_matchedid"][i]] != 0]
    return {"source": [int(pairs["source_matchedid"][i]) for i in keep], "target": [int(pairs["target_matchedid"][i]) for i in keep],
            "relevance": [float(pairs["score"][i]) for i in keep],
            "weight": [math.sqrt(float(pairs["source_popularity"][i])) for i in keep]}


def save_metrics(embeddings, pairs, testmasks, score_rows=None):
    """the `ret` dict of save_metrics.  score_rows[m] (optional): {source: masked score row} to rank instead of the restatement's own
    Float32 Gram matrix (the GPU tests pass the device's rows: the BLAS summation order of E' * E cannot be reproduced)"""
    ret = {}
    for medium in sorted(embeddings):
        df = metric_frame(pairs[medium], testmasks[medium], medium)
        M = score_rows[medium] if score_rows is not None else masked_gram(embeddings[medium], testmasks[medium])
        for k in KS:
            ret[f"{medium}.nDCG@{k}"] = ndcg_at_k(df, M, k)
            ret[f"{medium}.Recall@{k}"] = recall_at_k(df, M, k)
    return ret


def toy_catalogue(V, E, seed, n_sources, medium, density=0.3, max_targets=12):
    """a small medium: unit-norm export, symmetric test mask, pairs.{m}.csv columns with duplicated targets, repeated (source,
    popularity) groups, rows of other cliptypes, zero scores, and rows the test mask drops"""
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((V, E)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True).astype(np.float32)
    m = rng.random((V, V)) < density
    testmask = m | m.T
    cols = {k: [] for k in ("cliptype", "source_matchedid", "source_popularity", "target_matchedid", "score")}

    def add(c, s, p, t, sc):
        for k, v in zip(cols, (c, s, p, t, sc)):
            cols[k].append(v)
    sources = rng.choice(np.arange(1, V), n_sources, replace=False)
    for s in sources:
        pop = float(rng.integers(1, 1000))
        cand = np.flatnonzero(testmask[s])
        cand = cand[cand != s]
        n = int(rng.integers(1, max_targets + 1))
        for t in rng.choice(cand, min(n, len(cand)), replace=False) if len(cand) else []:
            add(f"medium{medium}", int(s), pop, int(t), float(rng.integers(1, 6)) / 2)
        if len(cand):
            add(f"medium{medium}", int(s), pop, int(cand[0]), 2.5)             # a repeated target: the last relevance wins
            add(f"medium{medium}", int(s), pop + 7.0, int(cand[-1]), 1.5)      # a second (source, popularity) group
            add(f"medium{medium}", int(s), pop, int(cand[0]), 0.0)             # dropped: score == 0
            add(f"adaptation{medium}", int(s), pop, int(cand[0]), 3.0)         # dropped: another cliptype
        out = np.flatnonzero(~testmask[s])
        if len(out):
            add(f"medium{medium}", int(s), pop, int(out[0]), 4.0)              # dropped: not a test pair
    pairs = {"cliptype": np.array(cols["cliptype"]), "source_matchedid": np.array(cols["source_matchedid"], np.int64),
             "source_popularity": np.array(cols["source_popularity"], np.float64),
             "target_matchedid": np.array(cols["target_matchedid"], np.int64), "score": np.array(cols["score"], np.float64)}
    return emb, testmask, pairs
