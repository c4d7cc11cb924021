"""Finetune/regress.jl on the device: the evaluation of a finetuned model over held-out users and the registry coefficients the serving
calls read (`{m}.retrieval.coefs`, `{m}.rating.coefs`, through serve._registry_coefs).

A test user is the dict of the reference's test msgpack files: "user", "items" (the list items, as `serve.predict` reads them) and
"test_items" (exactly one held-out item).  `regress_records` turns the users of one medium into regress.jl's records (`save_users`
without HTTP or JLD2); `regress_retrieval` / `regress_ranking` fit the coefficients; `retrieval_metrics` / `ranking_metrics` compute
HR@k, nDCG@k and the weighted ranking nDCG; `save_weights` runs them in regress.jl's order and returns the merged registry.

Every "score a medium's whole item table" step runs on the device: the top-k candidates through `rsys_retrieve_topk`, the target's rank
and log-probability through `rsys_retrieve_target_rank`, the candidates' ranking scores through `rsys_rank_request`.  Ranks follow
Julia's `partialsortperm(logp, rev=true)` order: descending score, ties by ascending id.

Deliberate differences from regress.jl:
* ranking_metrics ranks a user's candidates by lp + r (log retrieval probability plus the rating blend), the score of render.jl's
  `ranking` and of `rsys_rank_request`; regress.jl ranks by p .* exp.(r) in fp32.  The two orders are equal in exact arithmetic and
  can differ on fp32 ties.
* a retrieval target whose probability underflows to 0 in fp32 (log-probability -inf) counts as a miss for HR and nDCG.
* the least-squares fit of regress_ranking runs in fp64 (regress.jl solves it in fp32).
"""
import numpy as np

from . import serve

DELETED_STATUS, PLANNED_STATUS = 3, 5      # regress.jl:13-14
RETRIEVAL_KS = (8, 128, 1024)              # regress.jl:211
MAX_USERS_PER_CALL = 4096                  # users per rsys_rank_request / rsys_retrieve_topk call
NEG_LOG_EPS = -float(np.log(np.finfo(np.float64).eps))   # -log(eps(Float64)): the cross-entropy's cap


def last_status(items, medium):
    """regress.jl:87-94: {matchedid: status of the item's last list entry} over the items of `medium`"""
    out = {}
    for x in items:
        if int(x["medium"]) == int(medium):
            out[int(x["matchedid"])] = int(x["status"])
    return out


def excluded_ids(status):
    """the business rules of regress.jl:98-104 and 220-226 as medium-local ids: item 0 and every item whose last status is neither
    deleted (3) nor planned (5)"""
    return np.array(sorted({0} | {i for i, s in status.items() if s not in (DELETED_STATUS, PLANNED_STATUS)}), np.int32)


def skip_user(u, medium, task):
    """regress.jl:149-173"""
    if task == "retrieval":
        if u["medium"] != medium or not u["predict_watch"]:
            return True
        if u["matchedid"] == 0:
            return True
        s = u["last_status"].get(u["matchedid"])
        if s is not None and s not in (DELETED_STATUS, PLANNED_STATUS):
            return True              # don't recommend items the user has already watched
        return False
    if task == "ranking":
        if u["medium"] != medium or not u["predict_rating"]:
            return True
        return u["matchedid"] == 0
    raise AssertionError(task)


def _outcome(item):
    """the labels of regress.jl:128-140 from the held-out item"""
    predict_rating = item["rating"] > 0 and item["rating"] != item["history_rating"]
    inferred_watch = item["status"] == 0 and item["history_status"] is None
    new_watch = item["status"] > PLANNED_STATUS and (item["history_status"] is None or 0 < item["history_status"] <= PLANNED_STATUS)
    return bool(predict_rating), bool(inferred_watch or new_watch)


def _chunks(n, size):
    return [(a, min(n, a + size)) for a in range(0, n, size)]


def ranking_ids(model, queries, medium, exclude, num_ranking_items, targets):
    """regress.jl:95-110 per user: the first `num_ranking_items` ids of sortperm(logp, rev=true) with the excluded ids at -inf (the top
    k of rsys_retrieve_topk; when fewer items are admissible, the -inf ones follow in ascending id order, as Julia's stable sort puts
    them), then the target swapped in for the last id when it is absent."""
    Vm = model.config["vocab_sizes"][f"{int(medium)}_matchedid"]
    k = int(num_ranking_items)
    out = []
    for a, b in _chunks(len(queries), MAX_USERS_PER_CALL):
        ids, _, counts = model.retrieve_topk(np.asarray(queries[a:b], np.float32), medium, k, exclude=exclude[a:b])
        for j in range(b - a):
            idxs = ids[j, :counts[j]].astype(np.int64)
            if idxs.size < k:
                rest = np.setdiff1d(np.arange(Vm), idxs, assume_unique=True)
                idxs = np.concatenate([idxs, rest[:k - idxs.size]])
            t = int(targets[a + j])
            if t not in set(idxs.tolist()):
                idxs[-1] = t
            out.append(idxs)
    return out


def regress_records(model, users, medium, num_ranking_items=1024, batch=None):
    """`save_users` (regress.jl:60-147) for the test users of `medium`, without HTTP or JLD2: the retrieval embedding (serve.predict),
    the last status per item of the medium, the top `num_ranking_items` candidates with the target swapped in, the ranking prediction
    at those candidates (serve.predict, in forwards of at most S - S // 2 candidates; candidates are masked from each other, so the
    chunking does not change the values), and the record fields.  Users whose held-out item is of the other medium are left out.
    `batch`: users per retrieval forward (default the model's max_rows)."""
    m = int(medium)
    sel = []
    for u in users:
        assert len(u["test_items"]) == 1
        if int(u["test_items"][0]["medium"]) == m:
            sel.append(u)
    if not sel:
        return []
    batch = int(batch or getattr(model, "max_rows", 1))
    reqs = [dict(user=u["user"], items=u["items"], timestamp=u["test_items"][0]["history_max_ts"]) for u in sel]
    emb = []
    for a, b in _chunks(len(reqs), batch):
        emb += [np.asarray(e[f"{m}.retrieval"], np.float32) for e in serve.predict(model, reqs[a:b], "retrieval", m)]
    status = [last_status(u["items"], m) for u in sel]
    targets = [int(u["test_items"][0]["matchedid"]) for u in sel]
    idxs = ranking_ids(model, np.stack(emb), m, [excluded_ids(s) for s in status], num_ranking_items, targets)
    S = model.config["max_sequence_length"]
    max_user_len = S // 2
    chunk = S - max_user_len
    records = []
    for u, req, e, st, cand in zip(sel, reqs, emb, status, idxs):
        vals = []
        for c0 in range(0, cand.size, chunk):
            r = dict(req, ranking_items=[int(x) for x in cand[c0:c0 + chunk]])
            vals += serve.predict(model, [r], "ranking", m, max_user_len, chunk)[0][f"{m}.ranking"]
        item = u["test_items"][0]
        predict_rating, predict_watch = _outcome(item)
        records.append({
            f"{m}.retrieval": e, f"{m}.ranking": np.asarray(vals, np.float32), "ranking_matchedids": cand.astype(np.int64),
            "medium": int(item["medium"]), "matchedid": int(item["matchedid"]), "rating": float(item["rating"]),
            "predict_rating": predict_rating, "predict_watch": predict_watch, "status": int(item["status"]), "last_status": st,
            "num_tokens": len(serve.project(u["items"])),
        })
    return records


def _retrieval_users(records, m):
    return [u for u in records if not skip_user(u, m, "retrieval")]


def target_ranks(model, records, medium):
    """(rank, logp) of every record's target among the admissible items of `medium` (rsys_retrieve_target_rank, exclusions item 0 and
    the non-3 / non-5 last statuses); an empty pair for no records"""
    if not records:
        return np.zeros(0, np.int32), np.zeros(0, np.float32)
    q = np.stack([np.asarray(u[f"{medium}.retrieval"], np.float32) for u in records])
    t = np.array([u["matchedid"] for u in records], np.int32)
    return model.retrieve_target_rank(q, medium, t, exclude=[excluded_ids(u["last_status"]) for u in records])


def regress_retrieval(model, records, medium):
    """regress.jl:244-266: coefs [1]; cross-entropy = mean over the retrieval users of -log(max(p, eps(Float64))) with p the target's
    unmasked soft-max probability, i.e. min(-logp, -log(eps)); num_users"""
    m = int(medium)
    users = _retrieval_users(records, m)
    _, logp = target_ranks(model, users, m)
    ce = np.minimum(-logp.astype(np.float64), NEG_LOG_EPS)
    return {f"{m}.retrieval.coefs": np.array([1.0]), f"{m}.retrieval.crossentropy": float(ce.sum() / len(users)) if users else float("nan"),
            f"{m}.retrieval.num_users": float(len(users))}


def regress_ranking(records, registry, medium):
    """regress.jl:268-289: the least squares fit of rating ~ [rating_mean, r_masked at the target] over the ranking users (weights 1),
    in fp64; coefs, the weighted mse of the fit, num_users"""
    m = int(medium)
    users = [u for u in records if not skip_user(u, m, "ranking")]
    mean = float(np.float32(np.asarray(registry[f"{m}.rating_mean"]).reshape(-1)[0]))
    X = np.zeros((len(users), 2))
    y = np.zeros(len(users))
    for i, u in enumerate(users):
        pos = list(np.asarray(u["ranking_matchedids"]).tolist()).index(u["matchedid"])
        X[i] = (mean, float(np.float32(u[f"{m}.ranking"][pos])))
        y[i] = float(np.float32(u["rating"]))
    beta = np.linalg.lstsq(X, y, rcond=None)[0] if users else np.zeros(2)
    mse = float(np.sum((X @ beta - y) ** 2) / len(users)) if users else float("nan")
    return {f"{m}.rating.coefs": beta, f"{m}.rating.mse": mse, f"{m}.rating.num_users": float(len(users))}


def retrieval_metric_values(ranks, ks=RETRIEVAL_KS):
    """per-k (HR, nDCG) means of 1-based target ranks with one relevant item (idcg = 1); rank 0 (target not admissible) is a miss"""
    r = np.asarray(ranks, np.int64)
    out = {}
    for k in ks:
        hit = (r >= 1) & (r <= k)
        gain = np.where(hit, 1.0 / np.log2(np.maximum(r, 1) + 1.0), 0.0)
        out[k] = (float(hit.sum() / r.size), float(gain.sum() / r.size)) if r.size else (float("nan"), float("nan"))
    return out


def retrieval_metrics(model, records, medium):
    """regress.jl:193-242: HR@k and nDCG@k for k = 8, 128, 1024 over the retrieval users, from the target ranks of
    rsys_retrieve_target_rank (exclusions: item 0 and the non-3 / non-5 last statuses)"""
    m = int(medium)
    ranks, _ = target_ranks(model, _retrieval_users(records, m), m)
    ret = {}
    for k, (hr, ndcg) in retrieval_metric_values(ranks).items():
        ret[f"{m}.retrieval.HR@{k}"] = hr
        ret[f"{m}.retrieval.nDCG@{k}"] = ndcg
    return ret


def candidate_rank(scores, pos):
    """1-based position of candidate `pos` in descending score order, ties by candidate position (Julia's partialsortperm order)"""
    s = np.asarray(scores, np.float32)
    j = np.arange(s.size)
    return int(1 + np.sum(s > s[pos]) + np.sum((s == s[pos]) & (j < pos)))


def weighted_ndcg(ranks, w):
    """regress.jl:309-318 with one relevant item per user: sum of w_i / log2(rank_i + 1) over sum of w"""
    r = np.asarray(ranks, np.float64)
    w = np.asarray(w, np.float64)
    return float(np.sum(w / np.log2(r + 1.0)) / np.sum(w)) if np.sum(w) else float("nan")


def ranking_metrics(model, records, registry, medium):
    """regress.jl:291-331 over the retrieval users: each user's candidates (its ranking_matchedids) scored by rsys_rank_request with
    the registry's coefficients -- lp + r for the model, lp alone for the baseline -- the target's rank among them, then nDCG with
    k = the number of candidates, weighted by exp(rating) (0 for rating 0: wnDCG) and by 1 (nDCG)"""
    m = int(medium)
    users = _retrieval_users(records, m)
    rc, kc, mean = serve._registry_coefs(registry, m)
    ranks = {"model": [], "baseline": []}
    for a, b in _chunks(len(users), MAX_USERS_PER_CALL):
        sub = users[a:b]
        q = np.stack([np.asarray(u[f"{m}.retrieval"], np.float32) for u in sub])
        cand = [np.asarray(u["ranking_matchedids"], np.int64) for u in sub]
        rm = [np.asarray(u[f"{m}.ranking"], np.float32) for u in sub]
        pos = [int(np.flatnonzero(c == u["matchedid"])[0]) for c, u in zip(cand, sub)]
        _, r = model.rank_request(q, m, cand, r_masked=rm, retrieval_coef=rc, rating_coefs=kc, rating_mean=mean, rerank=False)
        _, p = model.rank_request(q, m, cand, r_masked=[np.zeros_like(x) for x in rm], retrieval_coef=rc, rerank=False)
        ranks["model"] += [candidate_rank(s, i) for s, i in zip(r, pos)]
        ranks["baseline"] += [candidate_rank(s, i) for s, i in zip(p, pos)]
    w_rating = [0.0 if u["rating"] == 0 else float(np.float32(np.exp(np.float64(np.float32(u["rating"]))))) for u in users]
    w_norating = [1.0] * len(users)
    return {
        f"{m}.ranking.wnDCG": weighted_ndcg(ranks["model"], w_rating),
        f"{m}.ranking.nDCG": weighted_ndcg(ranks["model"], w_norating),
        f"{m}.ranking.wnDCG.baseline": weighted_ndcg(ranks["baseline"], w_rating),
        f"{m}.ranking.nDCG.baseline": weighted_ndcg(ranks["baseline"], w_norating),
    }


def save_weights(model, users_by_medium, registry, num_ranking_items=1024):
    """regress.jl:380-411 without the CSV, the upload and JLD2: the records of both mediums first (`users_by_medium`: {medium: test
    users}, or one list of test users, each medium taking those whose held-out item is of it), then per medium the two regressions,
    merged into the registry, then both metric sets computed with the merged registry.  Returns the merged registry (a new dict)."""
    registry = dict(registry)
    pick = (lambda m: users_by_medium.get(m, [])) if isinstance(users_by_medium, dict) else (lambda m: users_by_medium)
    records = {m: regress_records(model, pick(m), m, num_ranking_items) for m in (0, 1)}
    for m in (0, 1):
        registry.update(regress_retrieval(model, records[m], m))
        registry.update(regress_ranking(records[m], registry, m))
        registry.update(retrieval_metrics(model, records[m], m))
        registry.update(ranking_metrics(model, records[m], registry, m))
    return registry
