"""numpy restatement of Finetune/regress.jl's evaluation (lines 175-331): `hitrate_at_k`, `ndcg_at_k`, `retrieval_metrics`,
`regress_retrieval`, `regress_ranking`, `weighted_ndcg` and `ranking_metrics`, the yardstick of recommendersystem_amd.regress.

Julia is not in the image: the forms are read from regress.jl's source, not pinned by running it.  `partialsortperm(p, rev=true, 1:k)`
is a full sort of the score row with Julia's `Perm` tie rule (equal scores by ascending index): np.lexsort on (index, -score); NaN never
occurs here and -Inf sorts last.  Records are the dicts of regress.regress_records (0-based ids); the retrieval log-probabilities come
in as given rows (`logp_rows`, one per record, over the medium's items), so the restatement does not need a model.
"""
import numpy as np

DELETED, PLANNED = 3, 5


def partialsortperm_rev(p, k):
    p = np.asarray(p, np.float64)
    idx = np.arange(p.size)
    return np.lexsort((idx, -p))[:k]


def hitrate_at_k(p, seen, k):
    return 1.0 if any(int(i) in seen for i in partialsortperm_rev(p, k)) else 0.0


def ndcg_at_k(p, seen, k):
    dcg = 0.0
    for rank, idx in enumerate(partialsortperm_rev(p, k), start=1):
        if int(idx) in seen:
            dcg += 1 / np.log2(rank + 1)
    max_hits = min(k, len(seen))
    idcg = sum(1 / np.log2(i + 1) for i in range(1, max_hits + 1))
    return 0.0 if idcg == 0 else dcg / idcg


def skip_user(u, medium, task):
    if task == "retrieval":
        if u["medium"] != medium or not u["predict_watch"]:
            return True
        if u["matchedid"] == 0:
            return True
        if u["matchedid"] in u["last_status"] and u["last_status"][u["matchedid"]] not in (DELETED, PLANNED):
            return True
        return False
    if task == "ranking":
        if u["medium"] != medium or not u["predict_rating"]:
            return True
        return u["matchedid"] == 0
    raise AssertionError(task)


def retrieval_metrics(users, logp_rows, medium, ks=(8, 128, 1024)):
    m = medium
    hitrate = {k: 0.0 for k in ks}
    ndcg = {k: 0.0 for k in ks}
    num_users = 0
    for u, row in zip(users, logp_rows):
        if skip_user(u, m, "retrieval"):
            continue
        logp = np.array(row, np.float64)
        logp[0] = -np.inf
        for x, s in u["last_status"].items():
            if s not in (DELETED, PLANNED):
                logp[x] = -np.inf
        ys = {u["matchedid"]}
        for k in ks:
            hitrate[k] += hitrate_at_k(logp, ys, k)
            ndcg[k] += ndcg_at_k(logp, ys, k)
        num_users += 1
    ret = {}
    for k in ks:
        ret[f"{m}.retrieval.HR@{k}"] = hitrate[k] / num_users
        ret[f"{m}.retrieval.nDCG@{k}"] = ndcg[k] / num_users
    return ret


def regress_retrieval(users, logp_target, medium):
    """logp_target: per user the log soft-max of its target (unmasked)"""
    m = medium
    p = np.zeros(len(users))
    y = np.zeros(len(users))
    for i, u in enumerate(users):
        if skip_user(u, m, "retrieval"):
            continue
        p[i] = np.exp(np.float64(logp_target[i]))
        y[i] = 1
    loss = np.sum(-np.log(np.maximum(p, np.finfo(np.float64).eps)) * y) / np.sum(y)
    return {f"{m}.retrieval.coefs": [1], f"{m}.retrieval.crossentropy": loss, f"{m}.retrieval.num_users": np.sum(y)}


def regress_ranking(users, registry, medium):
    m = medium
    n = len(users)
    x_baseline, x_masked, y, w = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for i, u in enumerate(users):
        if skip_user(u, m, "ranking"):
            continue
        x_baseline[i] = np.float32(registry[f"{m}.rating_mean"])
        x_masked[i] = u[f"{m}.ranking"][list(u["ranking_matchedids"]).index(u["matchedid"])]
        y[i] = u["rating"]
        w[i] = 1
    X = np.stack([x_baseline, x_masked], 1)
    beta = np.linalg.lstsq(X * np.sqrt(w)[:, None], y * np.sqrt(w), rcond=None)[0]
    loss = np.sum(w * (X @ beta - y) ** 2) / np.sum(w)
    return {f"{m}.rating.coefs": beta, f"{m}.rating.mse": loss, f"{m}.rating.num_users": np.sum(w)}


def weighted_ndcg(x, y, w):
    """x, y: (k, n) scores and 0/1 labels per user column; w: (n,) weights"""
    k, n = y.shape
    ndcg = 0.0
    for i in range(n):
        ys = set(np.flatnonzero(y[:, i] == 1).tolist())
        ndcg += ndcg_at_k(x[:, i], ys, k) * w[i]
    return ndcg / np.sum(w)


def ranking_metrics(users, lp_rows, r_rows, medium):
    """lp_rows / r_rows: per user the log retrieval probability and the rating blend at its ranking_matchedids; the score ranked is
    lp + r (model) and lp (baseline), regress.py's ranking score (regress.jl ranks p .* exp.(r), the same order in exact arithmetic)"""
    m = medium
    kept = [i for i, u in enumerate(users) if not skip_user(u, m, "retrieval")]
    k = len(users[kept[0]]["ranking_matchedids"])
    lp = np.zeros((k, len(kept)), np.float32)
    r = np.zeros((k, len(kept)), np.float32)
    y = np.zeros((k, len(kept)), np.int32)
    w = np.zeros(len(kept), np.float32)
    for c, i in enumerate(kept):
        u = users[i]
        y[list(u["ranking_matchedids"]).index(u["matchedid"]), c] = 1
        w[c] = u["rating"]
        lp[:, c] = lp_rows[i]
        r[:, c] = r_rows[i]
    w_rating = np.array([0 if x == 0 else np.exp(1.0) ** x for x in w], np.float32)
    w_norating = np.ones(len(w), np.float32)
    model = lp + r
    return {
        f"{m}.ranking.wnDCG": weighted_ndcg(model, y, w_rating),
        f"{m}.ranking.nDCG": weighted_ndcg(model, y, w_norating),
        f"{m}.ranking.wnDCG.baseline": weighted_ndcg(lp, y, w_rating),
        f"{m}.ranking.nDCG.baseline": weighted_ndcg(lp, y, w_norating),
    }
