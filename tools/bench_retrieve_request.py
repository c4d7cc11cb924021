"""Whole retrieval requests on the device (rsys_retrieve_request, render.jl `retrieval(state)`) against today's integration path:
the item-similarity prior and the relation masks in numpy on the host, then rsys_retrieve_topk with the uploaded dense prior and the
masked ids as exclusions (INTEGRATION.md before this change).

bf16 models at the cfg-3 (D = 512) and production (D = 2048) widths with V_0 = 120 000 / V_1 = 40 000, requests of the manga medium,
an fp32 item-similarity table of width 1024, 1 / 16 / 64 groups of 1-2 users with 200-1000 list items each, 0 / 4 selected items per
group (half of them of the other medium: the crossproject path), k = 1024.  The relation files are not public, so franchise-like
relations are synthesised (the density is an assumption): `dependencies` the transitive closure of chains of 1-20 items, `recaps`
symmetric pairs over 5 % of the items, `adaptations` links to 1-3 items of the other medium for 30 % of the items.

Device: wall time of the synchronous call (median of --reps after --warmup).  Host path: the numpy prior and masks (sparse products as
O(nnz) bincounts, as a CSC product costs) timed for at most --host-groups groups and scaled to the request's group count, plus the
measured rsys_retrieve_topk call with the dense prior upload and the exclusions.  One JSON line per case, all of them in --out.

    python tools/bench_retrieve_request.py --out profiles/retrieve_request_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V0, V1, DIM = 120000, 40000, 1024


def franchise_relations(rng, V):
    """{m}.dependencies / recaps / adaptations as 0-based CSC tuples (indptr, indices, data, shape)"""
    def csc(rows, cols, shape):
        key = np.unique(np.asarray(cols, np.int64) * shape[0] + np.asarray(rows, np.int64))
        c, r = key // shape[0], key % shape[0]
        indptr = np.zeros(shape[1] + 1, np.int64)
        indptr[1:] = np.cumsum(np.bincount(c, minlength=shape[1]))
        return indptr, r.astype(np.int32), np.ones(r.size, np.float32), shape

    rel = {}
    for m in (0, 1):
        n, no = V[m], V[1 - m]
        perm = rng.permutation(n)
        rows, cols, i = [], [], 0
        while i < n:                                  # chains: item j of a chain depends on every earlier item (transitive closure)
            L = int(rng.integers(1, 21))
            ch = perm[i:i + L]
            for a in range(1, ch.size):
                rows += [ch[a]] * a; cols += ch[:a].tolist()
            i += L
        rel[f"{m}.dependencies"] = csc(rows, cols, (n, n))
        pairs = rng.choice(n, size=(n // 40, 2), replace=True)
        pairs = pairs[pairs[:, 0] != pairs[:, 1]]
        rel[f"{m}.recaps"] = csc(np.r_[pairs[:, 0], pairs[:, 1]], np.r_[pairs[:, 1], pairs[:, 0]], (n, n))
        src = np.flatnonzero(rng.random(n) < 0.3)
        cnt = rng.integers(1, 4, src.size)
        rel[f"{m}.adaptations"] = csc(np.repeat(src, cnt), rng.integers(0, no, int(cnt.sum())), (n, no))
    return rel


def csc_matvec(A, x):
    indptr, indices, data, shape = A
    col = np.repeat(np.arange(shape[1]), np.diff(indptr))
    return np.bincount(indices, weights=data * x[col], minlength=shape[0])


def host_prior_and_mask(m, rel, sim, V, users, selected):
    """render.jl:241-331 on the host for one group: the float32 prior and the masked ids (the integration path before this change)"""
    Em = sim[f"embeddings.{m}"]                       # (dim, V_m)
    p = np.zeros(V[m], np.float32)
    for am, i in selected:
        x = sim[f"embeddings.{am}"][:, i]
        if am != m:
            x = sim[f"crossproject.{am}"] @ x
        p += Em.T @ x
    dep, rec, ada = (rel[f"{m}.{k}"] for k in ("dependencies", "recaps", "adaptations"))
    masked = np.zeros(V[m], bool)
    masked[0] = True
    ones = csc_matvec(dep, np.ones(V[m], np.float32)) != 0
    for items in users:
        st = {0: {}, 1: {}}
        for y, i, s in items:
            st[y][i] = s
        w = {y: np.zeros(V[y], np.float32) for y in (0, 1)}
        for y in (0, 1):
            for i, s in st[y].items():
                if s not in (3, 5):
                    w[y][i] = 1
        masked |= w[m] != 0
        masked |= (csc_matvec(ada, w[1 - m]) != 0) & (csc_matvec(dep, w[m]) == 0)
        masked |= csc_matvec(rec, w[m]) != 0
        c = np.zeros(V[m], np.float32); c[[i for i, s in st[m].items() if s >= 7]] = 1
        masked |= ones & (csc_matvec(dep, c) == 0)
        kk = np.zeros(V[m], np.float32); kk[[i for i, s in st[m].items() if s in (6, 2, 1)]] = 1
        masked |= csc_matvec(dep, kk) != 0
    for am, i in selected:
        if am == m:
            masked[i] = True
    return p, np.flatnonzero(masked)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg3,prod")
    ap.add_argument("--groups", default="1,16,64")
    ap.add_argument("--selected", default="0,4")
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-groups", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import recommendersystem_amd as ra
    from recommendersystem_amd import serve, workload
    rng = np.random.default_rng(1)
    V = (V0, V1)
    t0 = time.perf_counter()
    rel = franchise_relations(rng, V)
    sim = {f"embeddings.{m}": (rng.standard_normal((DIM, V[m])) / np.sqrt(DIM)).astype(np.float32) for m in (0, 1)}
    sim.update({f"crossproject.{m}": (rng.standard_normal((DIM, DIM)) / np.sqrt(DIM)).astype(np.float32) for m in (0, 1)})
    print(json.dumps({"setup_s": round(time.perf_counter() - t0, 1),
                      "nnz": {k: int(v[0][-1]) for k, v in rel.items()}}), flush=True)
    m = 0
    results = []
    for shape in a.shapes.split(","):
        cfg = workload.make_config(shape)
        cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"] = V
        model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=1)
        model.init_weights(7)
        model.random_pretrained_embeddings(8)
        serve.load_retrieval_tables(model, rel, sim)
        D = cfg["embed_dim"]
        F = model.item_embeddings()[:V0]
        scale = 4.0 / np.sqrt(D) / max(1e-6, float(np.abs(F).mean()))
        del F
        for ng in (int(x) for x in a.groups.split(",")):
            n_users = rng.integers(1, 3, ng)
            group = np.repeat(np.arange(ng, dtype=np.int32), n_users)
            q = (rng.standard_normal((group.size, D)) * scale).astype(np.float32)
            hist = []
            for _ in range(group.size):
                n = int(rng.integers(200, 1001))
                y = (rng.random(n) < 0.3).astype(np.int64)
                ids = np.where(y == 0, rng.integers(0, V0, n), rng.integers(0, V1, n))
                hist.append(list(zip(y.tolist(), ids.tolist(), rng.integers(0, 9, n).tolist())))
            for ns in (int(x) for x in a.selected.split(",")):
                sel = [[(j % 2, int(rng.integers(0, V[j % 2]))) for j in range(ns)] for _ in range(ng)]
                run = lambda: model.retrieve_request(q, m, a.k, group=group, histories=hist, selected=sel)
                for _ in range(a.warmup):
                    run()
                ts = []
                for _ in range(a.reps):
                    t1 = time.perf_counter()
                    out = run()
                    ts.append((time.perf_counter() - t1) * 1e3)
                # host path: prior + masks for a few groups (scaled), then retrieve_topk with the dense prior and the exclusions
                hg = min(ng, a.host_groups)
                t1 = time.perf_counter()
                parts = [host_prior_and_mask(m, rel, sim, V, [hist[u] for u in np.flatnonzero(group == g)], sel[g]) for g in range(hg)]
                host_prep_ms = (time.perf_counter() - t1) * 1e3 / hg * ng
                prior = np.stack([parts[g % hg][0] for g in range(ng)])
                excl = [parts[g % hg][1] for g in range(ng)]
                tt = []
                for _ in range(max(1, a.reps // 2)):
                    t1 = time.perf_counter()
                    model.retrieve_topk(q, m, a.k, group=group, prior=prior, exclude=excl)
                    tt.append((time.perf_counter() - t1) * 1e3)
                topk_ms = float(np.median(tt))
                # the same request's groups on the host path agree with the device where they were computed exactly (first hg)
                ok = None
                if hg:
                    ids_h, _, cnt_h = model.retrieve_topk(q[group < hg], m, a.k, group=group[group < hg],
                                                          prior=prior[:hg], exclude=excl[:hg])
                    ok = bool(all(len(set(out[0][g, :out[2][g]]) ^ set(ids_h[g, :cnt_h[g]])) <= max(2, a.k // 100) for g in range(hg)))
                r = {"shape": shape, "embed_dim": D, "V_m": V0, "V_other": V1, "sim_dim": DIM, "groups": ng, "users": int(group.size),
                     "list_items": int(sum(len(h) for h in hist)), "selected_per_group": ns, "k": a.k,
                     "device_ms_median": round(float(np.median(ts)), 3), "device_ms_min": round(float(np.min(ts)), 3),
                     "host_path_ms": round(host_prep_ms + topk_ms, 1), "host_prep_ms": round(host_prep_ms, 1),
                     "host_topk_with_prior_ms": round(topk_ms, 3), "host_groups_timed": hg, "same_candidates": ok}
                print(json.dumps(r), flush=True)
                results.append(r)
        model.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
