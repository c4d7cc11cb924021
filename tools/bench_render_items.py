"""What the windowed retrieval costs: rsys_render_items -- a page for states without users -- at offset 0 and at an
offset past rank 50 000, against the host restatement of the same page (render.jl in numpy: the fp32 prior, a stable argsort of the
whole medium, the reranking loop on the window); and rsys_retrieve_window for states with users against rsys_retrieve_request at
k = 8192, the call it stands in for when `serve.render(..., exact=True)` asks for a page's candidates (at rank 0 and at the deepest
full window below the states' totals).

V = 120 000 / 80 000, an fp32 item-similarity table of width 256, 1 / 16 / 64 states (media alternating; 2 selected items each, one of
the other medium: the crossproject path), limit 10.  A cfg-3-sized bf16 model carries the tables; the user-less path never reads its
item table.  States with users: 1-2 users of 300 list items each, synthetic relations as tools/bench_retrieve_request.py.  Host clock
around the synchronous call, warm, --reps repeats per path in three alternating blocks; median, quartiles and extremes per case
(DESIGN.md 4u's method).  One JSON line per case, all of them in --out.

    python tools/bench_render_items.py --out profiles/render_items_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

V = (120000, 80000)
DIM = 256
PEN = dict(decay=0.9, mmr_penalty=0.25, same_series_penalty=0.5, related_penalty=0.5)


def stats(ts):
    ts = np.asarray(ts) * 1e3
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    return {"median_ms": round(float(med), 3), "q1_ms": round(float(q1), 3), "q3_ms": round(float(q3), 3),
            "min_ms": round(float(ts.min()), 3), "max_ms": round(float(ts.max()), 3), "n": int(ts.size)}


def alternate(paths, reps, warmup):
    """{name: [seconds]}: every path warmed, then `reps` timed calls each in three alternating blocks"""
    for fn in paths.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in paths}
    for block in range(3):
        n = reps // 3 + (1 if block < reps % 3 else 0)
        for k, fn in paths.items():
            for _ in range(n):
                t0 = time.perf_counter()
                fn()
                out[k].append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="1,16,64")
    ap.add_argument("--deep-offset", type=int, default=50010)
    ap.add_argument("--limit", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import recommendersystem_amd as ra
    from recommendersystem_amd import serve, workload
    import _render_items_np as ri
    import _render_retrieval_np as rr
    from bench_retrieve_request import franchise_relations

    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    rel = franchise_relations(rng, V)
    sim = {f"embeddings.{m}": (rng.standard_normal((DIM, V[m])) / np.sqrt(DIM)).astype(np.float32) for m in (0, 1)}
    sim.update({f"crossproject.{m}": (rng.standard_normal((DIM, DIM)) / np.sqrt(DIM)).astype(np.float32) for m in (0, 1)})
    related = {f"{m}.related": rr.random_csc(rng, V[m], V[m], 8.0 / V[m]) for m in (0, 1)}
    cfg = workload.make_config("cfg3")
    cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"] = V
    model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=1)
    model.init_weights(7)
    model.random_pretrained_embeddings(8)
    serve.load_retrieval_tables(model, rel, sim)
    serve.load_ranking_tables(model, related)
    D = cfg["embed_dim"]
    print(json.dumps({"setup_s": round(time.perf_counter() - t0, 1), "V": V, "sim_dim": DIM, "embed_dim": D}), flush=True)
    results = []

    def emit(r):
        print(json.dumps(r), flush=True)
        results.append(r)

    for ng in (int(x) for x in a.groups.split(",")):
        # ---- states without users: one device call against the host restatement
        states = []
        for g in range(ng):
            m = g % 2
            items = [dict(medium=m, matchedid=int(rng.integers(1, V[m]))), dict(medium=1 - m, matchedid=int(rng.integers(1, V[1 - m])))]
            states.append(dict(medium=m, users=[], items=items, penalties=PEN))
        for name, offset in (("first page", 0), ("deep page", a.deep_offset)):
            pg = dict(offset=offset, limit=a.limit)
            ts = alternate({"device": lambda: serve.render_items(model, states, pg)}, a.reps, a.warmup)
            pages = serve.render_items(model, states, pg)
            hs = []
            for _ in range(a.host_reps):                        # the host path costs the same per state: time one, scale
                t1 = time.perf_counter()
                want = ri.render_literal(states[0], pg, sim, related, V)
                hs.append((time.perf_counter() - t1) * ng)
            # fp32 sums in another order may swap near-ties between device and host; the totals must agree, the pages usually do
            same = bool(np.array_equal(want[0], pages[0][0]))
            emit({"case": "render_items", "page": name, "states": ng, "offset": offset, "limit": a.limit,
                  "total_0": int(pages[0][1]), "page_ids": int(pages[0][0].size), "device": stats(ts["device"]),
                  "host_restatement_scaled": stats(hs), "host_states_timed": 1, "totals_equal": bool(want[1] == pages[0][1]),
                  "same_page_as_host": same})
        # ---- states with users: the window of a page against the top 8192
        m = 0
        n_users = rng.integers(1, 3, ng)
        group = np.repeat(np.arange(ng, dtype=np.int32), n_users)
        F = model.item_embeddings()[:V[0]]
        scale = 4.0 / np.sqrt(D) / max(1e-6, float(np.abs(F).mean()))
        del F
        q = (rng.standard_normal((group.size, D)) * scale).astype(np.float32)
        hist = []
        for _ in range(group.size):
            n = 300
            y = (rng.random(n) < 0.3).astype(np.int64)
            ids = np.where(y == 0, rng.integers(0, V[0], n), rng.integers(0, V[1], n))
            hist.append(list(zip(y.tolist(), ids.tolist(), rng.integers(0, 9, n).tolist())))
        sel = [[(0, int(rng.integers(1, V[0]))), (1, int(rng.integers(1, V[1])))] for _ in range(ng)]
        mitr = 1024 - 1024 % a.limit
        # the relation rules leave far fewer admissible items than V_m: the deepest full window below every state's total, which lies
        # past the cap of 8192 whenever the totals allow it
        totals = model.retrieve_window(q, m, [0] * ng, [1] * ng, group=group, histories=hist, selected=sel)[3]
        deep = max(0, min(a.deep_offset, int(totals.min()) - mitr)) // mitr * mitr
        paths = {"retrieve_request k=8192": lambda: model.retrieve_request(q, m, 8192, group=group, histories=hist, selected=sel),
                 "retrieve_window start=0": lambda: model.retrieve_window(q, m, [0] * ng, [mitr] * ng, group=group, histories=hist, selected=sel),
                 f"retrieve_window start={deep}": lambda: model.retrieve_window(q, m, [deep] * ng, [mitr] * ng, group=group, histories=hist,
                                                                                selected=sel)}
        ts = alternate(paths, a.reps, a.warmup)
        top = paths["retrieve_request k=8192"]()
        win = paths["retrieve_window start=0"]()
        emit({"case": "retrieve_window", "states": ng, "users": int(group.size), "window": mitr,
              **{k: stats(v) for k, v in ts.items()},
              "window_is_the_top_slice": bool(win[0][:, :mitr].tobytes() == top[0][:, :mitr].tobytes()),
              "deep_start": deep, "total_min": int(totals.min()), "total_max": int(totals.max())})
    model.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
