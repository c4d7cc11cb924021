"""Ranking and reranking of a page's candidates on the device (rsys_rank_request: render.jl `ranking` + `reranking!`) against the host
path it replaces: numpy `compute_retrieval` (a soft-max over the medium's whole item table per user) and the restatement of the greedy
loop with the Gram matrix `embs' * embs` in float32 (tests/_render_rank_np.py).

bf16 models at the cfg-3 (D = 512) and production (D = 2048) widths with V_0 = 120 000 / V_1 = 40 000, requests of the manga medium,
an fp32 item-similarity table of width 1024, n = 1024 candidates per group, one user per group with 300 list items, 1 / 16 / 64 groups,
partialk 25 (a first page) and 1024 (the whole slice).  "{m}.related" is synthesised (franchises of 1-20 items, every pair related).

Device columns: the whole call, the ranking score alone (rerank=False: score GEMM, log-sum-exp, combine), the Gram kernel alone
(rsys_rank_gram_get, including its copy of the n x n matrices to the host), the loop as the remainder, and the host-side packing of
the request (serve.rank_arrays).  Wall times, median of --reps after --warmup.  The host path is timed for one group and scaled.

    python tools/bench_rank_request.py --out profiles/rank_request_bench.json
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

V0, V1, DIM, N = 120000, 40000, 1024, 1024


def franchise_related(rng, n):
    perm = rng.permutation(n)
    rows, cols, i = [], [], 0
    while i < n:
        L = int(rng.integers(1, 21))
        ch = perm[i:i + L]
        rows.append(np.repeat(ch, ch.size)); cols.append(np.tile(ch, ch.size))
        i += L
    key = np.unique(np.concatenate(cols).astype(np.int64) * n + np.concatenate(rows))
    c, r = key // n, key % n
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(c, minlength=n))
    return indptr, r.astype(np.int32), np.ones(r.size, np.float32), (n, n)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg3,prod")
    ap.add_argument("--groups", default="1,16,64")
    ap.add_argument("--partialk", default="25,1024")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import _render_rank_np as rk
    import recommendersystem_amd as ra
    from recommendersystem_amd import serve, workload
    rng = np.random.default_rng(1)
    V = (V0, V1)
    related = {f"{m}.related": franchise_related(rng, V[m]) for m in (0, 1)}
    sim = {f"embeddings.{m}": (rng.standard_normal((DIM, V[m])) / np.sqrt(DIM)).astype(np.float32) for m in (0, 1)}
    m = 0
    results = []
    for shape in a.shapes.split(","):
        cfg = workload.make_config(shape)
        cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"] = V
        model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=1)
        model.init_weights(7)
        model.random_pretrained_embeddings(8)
        serve.load_retrieval_tables(model, {}, sim)
        serve.load_ranking_tables(model, related)
        D = cfg["embed_dim"]
        F = model.item_embeddings()[:V0]
        for ng in (int(x) for x in a.groups.split(",")):
            states, idxs = [], []
            for _ in range(ng):
                items = [dict(medium=int(rng.integers(0, 2)), matchedid=int(rng.integers(0, V1)), status=int(rng.integers(0, 9)))
                         for _ in range(300)]
                u = {"user": {"items": items}, "embeds": {"0.retrieval": (rng.standard_normal(D) / np.sqrt(D)).astype(np.float32),
                                                          "0.ranking": rng.uniform(0, 10, N).astype(np.float32)}}
                states.append(dict(medium=m, users=[u], penalties=dict(decay=0.9, mmr_penalty=0.5, same_series_penalty=1.0,
                                                                       related_penalty=0.5)))
                idxs.append(rng.choice(V0, N, replace=False).astype(np.int32))
            t_pack = timed(lambda: serve.rank_arrays(states, idxs), 1, 3)
            q, group, rm, hist, pen = serve.rank_arrays(states, idxs)
            t_rank = timed(lambda: model.rank_request(q, m, idxs, group=group, r_masked=rm, rerank=False), a.warmup, a.reps)
            t_gram = timed(lambda: model.rank_gram(m, idxs), a.warmup, a.reps)
            # host path of one group: compute_retrieval + compute_ranking on the host, then reranking! restated
            reg = {"0.watch.weight": F, "0.rating_mean": 3.0}
            st, c = states[0], idxs[0]

            def host_one(pk):
                u = st["users"][0]["embeds"]
                p = serve.compute_retrieval(reg, 0, u, c)
                with np.errstate(divide="ignore"):
                    r = np.log(p) + serve.compute_ranking(reg, 0, u)
                return rk.reranking(st, c, r.astype(np.float32), pk, related["0.related"], sim["embeddings.0"].T)

            for pk in (int(x) for x in a.partialk.split(",")):
                t_full = timed(lambda: model.rank_request(q, m, idxs, group=group, r_masked=rm, partialk=[pk] * ng, penalties=pen,
                                                          histories=hist), a.warmup, a.reps)
                t_host1 = timed(lambda: host_one(pk), 0, 1)
                res = dict(shape=shape, D=D, groups=ng, n=N, partialk=pk, dim=DIM, device_ms=round(t_full, 3),
                           device_rank_only_ms=round(t_rank, 3), device_gram_with_copy_ms=round(t_gram, 3),
                           loop_and_pairs_ms_est=round(max(0.0, t_full - t_rank - t_gram), 3), host_packing_ms=round(t_pack, 3),
                           host_path_ms=round(t_host1 * ng, 1), host_path_one_group_ms=round(t_host1, 1))
                results.append(res)
                print(json.dumps(res), flush=True)
        model.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
