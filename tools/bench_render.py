"""A page from raw histories: serve.render_users (one rsys_render_request call: both forwards, retrieval, ranking and reranking chained
on the device) against the staged sequence it replaces -- one serve.predict per user for the "{m}.retrieval" embedding, then
serve.render (retrieval -> host, one single-row ranking forward per user and chunk, rank_request).  Both run on the same model in the
same process; the staged functions are the ones of the commit before rsys_render_request existed, unchanged.

The cfg-3-sized inference model with S = 1024 (ranking rows hold 512 candidates: a 1024-candidate page is two chunks per user), bf16, a
four-adapter bank, max_rows 4; V_0 = 120 000 / V_1 = 80 000, item-similarity width 256, sparse random relations, users with 300 list
events.  Cases: (a) 1 user, first page of 10; (b) 3 users of one state; (c) 8 states of mixed media (1-3 users each) in one call.
Wall time per request (host clock around the synchronous call, which is what a server waits for): median of --reps after --warmup
with the quartiles and the extremes of the repeats; the two paths are timed in alternating blocks so that drift hits both.  Forwards
are counted (the staged path: calls of inference_select; the new path: the library's counter).  Bytes and host<->device copies are
NOT intercepted at the runtime: they are computed from the arrays each path hands to / receives from the library and from the copy
calls at the call sites of the entry points involved (per forward: 1 batch blob + selection [+ adapter rows] up, 1 result down;
retrieve_request: 7 up, 3 down; rank_request: 10 up, 2 down; render_request: per retrieval wave blob + selection [+ adapter rows], per
medium what the two request bodies upload minus queries / candidates / r_masked, 10 prefix arrays once, per ranking wave descriptors
[+ adapter rows]; down: counts per medium and the pages).

    python tools/bench_render.py --out profiles/render_request_bench.json

--full-history: the same set-up, three paths timed in the same process in alternating blocks -- (i) the staged
full-history path (one serve.predict per user, then serve.render(..., full_history=True): unchanged code), (ii)
serve.render_users(full_history=True) (one rsys_render_request_full call), (iii) serve.render_users() -- for users with --events and
with 1000 events.  Forwards of (i) are counted at the wrapper (inference_select, rank_cache_store, rank_cache_candidates), of (ii) / (iii)
by the library and compared with serve.render_full_forwards.  "bytes up" of (ii) is (iii)'s accounting minus the prefix arrays.

    python tools/bench_render.py --full-history --out profiles/render_full_bench.json

--weights: serve.render_users alone on the same set-up and cases, two arms in alternating blocks -- the states as they
are (no "weight" key: rsys_query_weights_set is never called, the unweighted kernels run) and the same states with a non-trivial weight
on every user and, in case (c), on two selected items of the state's medium per state (the weighted kernels).  One JSON line per case.  On a tree without
query weights only the unweighted arm runs, so the same command measures the commit before for an A/B across builds.

    python tools/bench_render.py --weights --out profiles/query_weights_bench.json

--texts: serve.render_users alone on the same set-up and cases, arms in alternating blocks -- the states as they are
(no "texts" key: rsys_query_texts_set is never called), and the same states with 1 and with 4 text queries per state, scored through a
search handle per medium on the model's item tables (Q = 3072; the setter's scoring is inside the timed call, as a server pays it).  On a
tree without text queries only the first arm runs, so the same command measures the commit before for an A/B across builds.

    python tools/bench_render.py --texts --out profiles/query_texts_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DIM = 256


def sparse_csc(rng, n_rows, n_cols, per_col):
    """a random 0-based CSC with about per_col entries per column"""
    counts = rng.poisson(per_col, n_cols)
    indptr = np.zeros(n_cols + 1, np.int64)
    indptr[1:] = np.cumsum(counts)
    rows = rng.integers(0, n_rows, int(indptr[-1])).astype(np.int32)
    for c in np.flatnonzero(counts > 1):                           # distinct rows inside a column
        seg = np.unique(rows[indptr[c]:indptr[c + 1]])
        rows[indptr[c]:indptr[c] + seg.size] = seg
        rows[indptr[c] + seg.size:indptr[c + 1]] = seg[-1]
    return indptr, rows, np.ones(rows.size, np.float32), (n_rows, n_cols)


def make_user(rng, V, n_events):
    items, ts = [], 1.2e9
    for _ in range(n_events):
        ts += float(rng.integers(10, 10 ** 6))
        y = int(rng.integers(0, 2))
        items.append({"medium": y, "matchedid": int(rng.integers(1, V[y])), "history_max_ts": ts, "status": int(rng.integers(0, 9)),
                      "rating": float(rng.integers(0, 11)), "progress": float(rng.random()), "history_status": -1, "history_rating": -1.0})
    return {"user": {"user": {"gender": None, "source": 2}, "items": items, "timestamp": ts + 60.0}}


def make_state(rng, V, m, n_users, events):
    return dict(medium=m, items=[], users=[make_user(rng, V, events) for _ in range(n_users)],
                penalties=dict(decay=0.9, mmr_penalty=0.5, same_series_penalty=1.0, related_penalty=0.5))


def stats(ts):
    ts = np.asarray(ts) * 1e3
    q1, q3 = np.percentile(ts, [25, 75])
    return dict(median_ms=round(float(np.median(ts)), 3), q1_ms=round(float(q1), 3), q3_ms=round(float(q3), 3),
                min_ms=round(float(ts.min()), 3), max_ms=round(float(ts.max()), 3), reps=int(ts.size))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="cfg3")
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--events", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--full-history", action="store_true", help="time the staged full-history path, render_users(full_history=True) and render_users()")
    ap.add_argument("--weights", action="store_true", help="time render_users without and with query weights (no staged path)")
    ap.add_argument("--texts", action="store_true", help="time render_users without text queries and with 1 and 4 per state (no staged path)")
    a = ap.parse_args()
    import recommendersystem_amd as ra
    from recommendersystem_amd import serve, workload
    rng = np.random.default_rng(1)
    cfg = workload.make_config(a.shape)
    cfg["max_sequence_length"] = a.seq
    cfg["forward"] = "inference"
    cfg["finetune"] = False
    V = (cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"])
    model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=4)
    model.init_weights(7)
    model.random_pretrained_embeddings(8)
    model.adapter_slots = {}
    for slot, key in enumerate(("0.retrieval", "0.ranking", "1.retrieval", "1.ranking")):
        model.load_adapter(slot, {n: (0.02 * rng.standard_normal(shape)).astype(np.float32) for n, shape in model.adapter_names()})
        model.adapter_slots[key] = slot
    rel = {}
    for m in (0, 1):
        rel[f"{m}.dependencies"] = sparse_csc(rng, V[m], V[m], 0.05)
        rel[f"{m}.recaps"] = sparse_csc(rng, V[m], V[m], 0.02)
        rel[f"{m}.adaptations"] = sparse_csc(rng, V[m], V[1 - m], 0.05)
    sim = {f"embeddings.{m}": (rng.standard_normal((DIM, V[m])) / np.sqrt(DIM)).astype(np.float32) for m in (0, 1)}
    serve.load_retrieval_tables(model, rel, sim)
    serve.load_ranking_tables(model, {f"{m}.related": sparse_csc(rng, V[m], V[m], 3.0) for m in (0, 1)})
    registry = {f"{m}.rating.coefs": np.array([0.3, 0.8]) for m in (0, 1)}
    registry.update({f"{m}.rating_mean": 4.0 for m in (0, 1)})
    pag = {"offset": 0, "limit": 10}
    cases = {"a_1_user": [make_state(rng, V, 0, 1, a.events)],
             "b_3_users": [make_state(rng, V, 0, 3, a.events)],
             "c_8_states": [make_state(rng, V, g % 2, 1 + g % 3, a.events) for g in range(8)]}

    # the staged path's traffic, counted at the wrapper: every array handed to / returned by the library
    counter = dict(forwards=0, up=0, down=0, copies=0)
    real_select, real_ret, real_rank = model.inference_select, model.retrieve_request, model.rank_request

    def count_select(d, task, token_index, adapters=None):
        out = real_select(d, task, token_index, adapters=adapters)
        n = int(np.asarray(d["userid"]).size)
        counter["forwards"] += 1
        counter["up"] += n * (9 * 4 + 8 + 18 * 4 + 8) + 4 * len(token_index); counter["down"] += out.nbytes; counter["copies"] += 3 + (adapters is not None)
        return out

    def count_ret(q, *p, **kw):
        out = real_ret(q, *p, **kw)
        counter["up"] += np.asarray(q).nbytes + sum(12 * len(h) for h in kw.get("histories") or [])
        counter["down"] += sum(x.nbytes for x in out); counter["copies"] += 10
        return out

    def count_rank(q, m, cand, **kw):
        out = real_rank(q, m, cand, **kw)
        counter["up"] += np.asarray(q).nbytes + sum(4 * len(c) for c in cand) * 3 + sum(np.asarray(r).nbytes for r in kw.get("r_masked") or []) \
            + sum(12 * len(h) for h in kw.get("histories") or [])
        counter["down"] += sum(4 * len(c) for c in cand); counter["copies"] += 12
        return out

    def staged(states):
        for st in states:
            m = int(st["medium"])
            for u in st["users"]:
                u["embeds"] = {f"{m}.retrieval": serve.predict(model, [u["user"]], "retrieval", m)[0][f"{m}.retrieval"]}
        return serve.render(model, states, pag, registry)

    results = []
    if a.full_history:
        results = full_history_cases(a, model, V, registry, pag, rng)
        cases = {}
    if a.weights:
        results = weights_cases(a, model, V, registry, pag, cases, rng)
        cases = {}
    if a.texts:
        results = texts_cases(a, model, cfg, V, registry, pag, cases, rng)
        cases = {}
    for name, states in cases.items():
        n_users = sum(len(st["users"]) for st in states)
        model.inference_select, model.retrieve_request, model.rank_request = count_select, count_ret, count_rank
        for k in counter:
            counter[k] = 0
        want = staged(states)
        staged_counts = dict(counter)
        model.inference_select, model.retrieve_request, model.rank_request = real_select, real_ret, real_rank
        got = serve.render_users(model, states, pag, registry)
        fw = model.render_kept("forwards").tolist()
        args = serve.render_pack(states, pag, a.seq, V[0], registry, model.adapter_slots)
        S = a.seq
        up = n_users * S * (9 * 4 + 8 + 18 * 4 + 8) + sum(v.nbytes for v in args["ranking_prefix"].values()) \
            + 2 * sum(12 * len(h) for h in args["histories"]) + n_users * (4 + 16 + 8)
        down = sum(p.nbytes for p, _ in got) + 2 * 4 * len(states)
        same = all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(want, got))
        t_staged, t_new = [], []
        blocks = 3
        for b in range(blocks):                                              # alternating blocks: staged, new, staged, new, ...
            t_staged += timed(lambda: staged(states), a.warmup if b == 0 else 1, a.reps // blocks)
            t_new += timed(lambda: serve.render_users(model, states, pag, registry), a.warmup if b == 0 else 1, a.reps // blocks)
        media = len({int(st["medium"]) for st in states})
        rmax = model.max_rows
        copies_new = -(-n_users // rmax) * 3 + media * (7 + 1) + 10 + -(-fw[1] // 1) * 2 + media * (8 + 3) + media
        res = dict(case=name, shape=a.shape, S=S, states=len(states), users=n_users, totals=[int(t) for _, t in got], same_pages=bool(same),
                   staged=dict(stats(t_staged), forwards=staged_counts["forwards"], bytes_up=staged_counts["up"],
                               bytes_down=staged_counts["down"], copies=staged_counts["copies"]),
                   render_users=dict(stats(t_new), forwards=sum(fw), forwards_retrieval=fw[0], forwards_ranking=fw[1], bytes_up=int(up),
                                     bytes_down=int(down), copies=int(copies_new)),
                   ratio_staged_over_new=round(float(np.median(t_staged) / np.median(t_new)), 3))
        results.append(res)
        print(json.dumps(res), flush=True)
    model.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


def weights_cases(a, model, V, registry, pag, cases, rng):
    """render_users on the states as they are against the same states with a weight on every user (and on the selected items that
    case (c) gets here: the other cases keep none, as their states have none)"""
    import copy
    from recommendersystem_amd import serve
    have = hasattr(serve, "state_weights")
    results = []
    for name, states in cases.items():
        if name == "c_8_states":
            for st in states:
                st["items"] = [dict(medium=int(st["medium"]), matchedid=int(rng.integers(1, V[int(st["medium"])]))) for _ in range(2)]
        weighted = copy.deepcopy(states)
        pool = [0.5, 2.25, -1.0, 3e-3, 1.5]
        for i, e in enumerate([u for st in weighted for u in st["users"]] + [x for st in weighted for x in st["items"]]):
            e["weight"] = pool[i % len(pool)]
        arms = {"unweighted": states}
        if have:
            arms["weighted"] = weighted
        t = {k: [] for k in arms}
        got = {k: serve.render_users(model, v, pag, registry) for k, v in arms.items()}
        blocks = 5
        for b in range(blocks):
            for k, v in arms.items():
                t[k] += timed(lambda: serve.render_users(model, v, pag, registry), a.warmup if b == 0 else 1, max(a.reps // blocks, 1))
        res = dict(case=name, shape=a.shape, S=a.seq, states=len(states), users=sum(len(st["users"]) for st in states),
                   selected=sum(len(st["items"]) for st in states), totals=[int(x) for _, x in got["unweighted"]],
                   **{k: stats(v) for k, v in t.items()})
        if have:
            res["pages_differ"] = bool(any(not np.array_equal(x[0], y[0]) for x, y in zip(got["unweighted"], got["weighted"])))
            res["weighted_over_unweighted"] = round(float(np.median(t["weighted"]) / np.median(t["unweighted"])), 4)
        results.append(res)
        print(json.dumps(res), flush=True)
    return results


def texts_cases(a, model, cfg, V, registry, pag, cases, rng):
    """render_users on the states as they are against the same states with 1 and with 4 text queries each"""
    import copy
    from recommendersystem_amd import search, serve
    have = hasattr(serve, "state_texts")
    S, Q = {}, 3072
    if have:
        W = (rng.standard_normal((Q, cfg["embed_dim"]), dtype=np.float32) * 1.5 / np.sqrt(Q)).astype(np.float32)
        for m in (0, 1):
            S[m] = search.SearchModel(search.training_config({m: V[m]}, batch_size=64, embed_dim=cfg["embed_dim"], query_dim=Q), m, model,
                                      dtype="bf16", max_batch=64)
            S[m].param_set("encoder.weight", W)
            S[m].param_set("logit_scale", 1.0)
    results = []
    for name, states in cases.items():
        arms = {"no_texts": states}
        for n in (1, 4) if have else ():
            arms[f"texts_{n}"] = copy.deepcopy(states)
            for st in arms[f"texts_{n}"]:
                st["texts"] = [{"embedding": rng.standard_normal(Q, dtype=np.float32), "weight": [1.0, 0.5, -1.0, 2.0][i]} for i in range(n)]
        kw = dict(search=S) if have else {}
        t = {k: [] for k in arms}
        got = {k: serve.render_users(model, v, pag, registry, **kw) for k, v in arms.items()}
        blocks = 5
        for b in range(blocks):
            for k, v in arms.items():
                t[k] += timed(lambda: serve.render_users(model, v, pag, registry, **kw), a.warmup if b == 0 else 1, max(a.reps // blocks, 1))
        res = dict(case=name, shape=a.shape, S=a.seq, states=len(states), users=sum(len(st["users"]) for st in states),
                   totals=[int(x) for _, x in got["no_texts"]], **{k: stats(v) for k, v in t.items()})
        for k in arms:
            if k != "no_texts":
                res[f"{k}_pages_differ"] = bool(any(not np.array_equal(x[0], y[0]) for x, y in zip(got["no_texts"], got[k])))
                res[f"{k}_over_no_texts"] = round(float(np.median(t[k]) / np.median(t["no_texts"])), 4)
        results.append(res)
        print(json.dumps(res), flush=True)
    for s in S.values():
        s.close()
    return results


def full_history_cases(a, model, V, registry, pag, rng):
    from recommendersystem_amd import serve
    S = a.seq
    results = []
    calls = dict(n=0)
    real = {k: getattr(model, k) for k in ("inference_select", "rank_cache_store", "rank_cache_candidates")}

    def counted(fn):
        def f(*p, **kw):
            calls["n"] += 1
            return fn(*p, **kw)
        return f

    def staged(states):
        for st in states:
            m = int(st["medium"])
            for u in st["users"]:
                u["embeds"] = {f"{m}.retrieval": serve.predict(model, [u["user"]], "retrieval", m)[0][f"{m}.retrieval"]}
        return serve.render(model, states, pag, registry, full_history=True)

    for events in sorted({a.events, 1000}):
        cases = {"a_1_user": [make_state(rng, V, 0, 1, events)], "b_3_users": [make_state(rng, V, 0, 3, events)],
                 "c_8_states": [make_state(rng, V, g % 2, 1 + g % 3, events) for g in range(8)]}
        for name, states in cases.items():
            n_users = sum(len(st["users"]) for st in states)
            for k, fn in real.items():
                setattr(model, k, counted(fn))
            calls["n"] = 0
            want = staged(states)
            staged_forwards = calls["n"]
            for k, fn in real.items():
                setattr(model, k, fn)
            got = serve.render_users(model, states, pag, registry, full_history=True)
            fw, ff = model.render_kept("forwards").tolist(), model.render_kept("forwards.full").tolist()
            split = serve.render_users(model, states, pag, registry)
            fw_split = model.render_kept("forwards").tolist()
            # the plan's forwards: users in r_masked order (medium 0's states, then medium 1's), every state has a page here
            order = [u for m in (0, 1) for st, (_, total) in zip(states, got) if int(st["medium"]) == m and total for u in st["users"]]
            nh = [len(serve._history(u["user"], S)) for u in order]
            nc = [min(1024 - 1024 % pag["limit"], total) for m in (0, 1) for st, (_, total) in zip(states, got)
                  if int(st["medium"]) == m and total for _ in st["users"]]
            plan = list(serve.render_full_forwards(nh, nc, S, model.max_rows))
            args = serve.render_pack(states, pag, S, V[0], registry, model.adapter_slots)
            prefix = sum(v.nbytes for v in args["ranking_prefix"].values())
            up_split = n_users * S * (9 * 4 + 8 + 18 * 4 + 8) + prefix + 2 * sum(12 * len(h) for h in args["histories"]) + n_users * (4 + 16 + 8)
            t = {"staged_full": [], "render_users_full": [], "render_users": []}
            fns = {"staged_full": lambda: staged(states), "render_users_full": lambda: serve.render_users(model, states, pag, registry, full_history=True),
                   "render_users": lambda: serve.render_users(model, states, pag, registry)}
            blocks = 3
            for b in range(blocks):
                for k in t:
                    t[k] += timed(fns[k], a.warmup if b == 0 else 1, a.reps // blocks)
            med = {k: float(np.median(v)) for k, v in t.items()}
            iqr_staged = float(np.subtract(*np.percentile(t["staged_full"], [75, 25])))
            res = dict(case=name, events=events, shape=a.shape, S=S, states=len(states), users=n_users, totals=[int(x) for _, x in got],
                       same_pages_as_staged=bool(all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(want, got))),
                       same_pages_as_split=bool(all(np.array_equal(x[0], y[0]) for x, y in zip(split, got))),
                       staged_full=dict(stats(t["staged_full"]), forwards=staged_forwards),
                       render_users_full=dict(stats(t["render_users_full"]), forwards=sum(fw), forwards_retrieval=fw[0], forwards_store=ff[0],
                                              forwards_candidates=ff[1], forwards_empty=ff[2], plan=plan, forwards_equal_plan=bool(ff == plan),
                                              bytes_up=int(up_split - prefix)),
                       render_users=dict(stats(t["render_users"]), forwards=sum(fw_split), bytes_up=int(up_split), prefix_bytes=int(prefix)),
                       full_below_staged_by_more_than_iqr=bool(med["staged_full"] - med["render_users_full"] > iqr_staged),
                       ratio_staged_over_full=round(med["staged_full"] / med["render_users_full"], 3),
                       full_over_split_ms=round((med["render_users_full"] - med["render_users"]) * 1e3, 3))
            results.append(res)
            print(json.dumps(res), flush=True)
    return results


if __name__ == "__main__":
    main()
