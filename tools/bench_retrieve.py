"""Retrieval top-k on the device (rsys_retrieve_topk) against the host path it replaces (serve.compute_retrieval + argsort).

bf16 models at the cfg-3 (D = 512) and production (D = 2048) widths, the manga medium (V_0 = 120 000), 1 / 16 / 64 users (one group
each), k = 1024 and 8192.  Device: wall time of the synchronous call on the host clock (median of --reps after --warmup calls).
Host: compute_retrieval (fp64 product over the registry table) + a stable argsort per user, timed on the same queries for at most
--host-users users and scaled to the request's user count (the per-user cost is independent of the others).  Prints one JSON line per
case and writes them to --out.

    python tools/bench_retrieve.py --out profiles/retrieve_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg3,prod")
    ap.add_argument("--users", default="1,16,64")
    ap.add_argument("--ks", default="1024,8192")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-users", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import recommendersystem_amd as ra
    from recommendersystem_amd import serve, workload
    results = []
    for shape in a.shapes.split(","):
        cfg = workload.make_config(shape)
        model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=1)
        model.init_weights(7)
        model.random_pretrained_embeddings(8)
        D, n0 = cfg["embed_dim"], cfg["vocab_sizes"]["0_matchedid"]
        registry = {"0.watch.weight": model.item_embeddings()[:n0]}
        rng = np.random.default_rng(1)
        Q = rng.standard_normal((max(int(u) for u in a.users.split(",")), D)).astype(np.float32)
        # queries of trunk-output scale against this table: logits with a spread of a few units
        Q *= 4.0 / np.sqrt(D) / max(1e-6, float(np.abs(registry["0.watch.weight"]).mean()))
        for n in (int(u) for u in a.users.split(",")):
            q = Q[:n]
            hn = min(n, a.host_users)
            t0 = time.perf_counter()
            for i in range(hn):
                p = serve.compute_retrieval(registry, 0, {"0.retrieval": q[i]})
                np.argsort(-p, kind="stable")
            host_ms = (time.perf_counter() - t0) * 1e3 / hn * n
            for k in (int(x) for x in a.ks.split(",")):
                for _ in range(a.warmup):
                    model.retrieve_topk(q, 0, k)
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    model.retrieve_topk(q, 0, k)
                    ts.append((time.perf_counter() - t0) * 1e3)
                r = {"shape": shape, "embed_dim": D, "V_m": n0, "users": n, "k": k, "device_ms_median": round(float(np.median(ts)), 4),
                     "device_ms_min": round(float(np.min(ts)), 4), "host_ms": round(host_ms, 2), "host_users_timed": hn,
                     "table_mb_bf16": round(n0 * D * 2 / 1e6, 1)}
                print(json.dumps(r), flush=True)
                results.append(r)
        model.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
