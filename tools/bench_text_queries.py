"""Times the scoring of a request's text queries (rsys_query_texts_set, DESIGN.md 4zg: upload, P = x Wenc, text_scores_kernel, the
log-sum-exp launches, one wait) at n = 1, 4, 8, 16 texts against the score stages of rsys_search_topk on the same handle and in the same
process: the forward-only evaluation call (upload, the same projection, the 256-row score GEMM into the fp32 slab, the row statistics;
no selection) and rsys_search_topk(k = 1) whole (those stages, the in-place log-probabilities and the selection).  A prod-sized
inference model with --layers trunk layers (default 1: the item tables do not depend on the depth) supplies the item tables (V_0 =
120 000, V_1 = 80 000, D = 2048), Q = 3072, bf16.  Host clock around the synchronous
calls, the three arms in alternating blocks; median and quartiles per arm.  One JSON line per (V_m, n), all of them to --out.

    python tools/bench_text_queries.py --out profiles/text_queries_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ts):
    ts = np.asarray(ts) * 1e3
    q1, q3 = np.percentile(ts, [25, 75])
    return dict(median_ms=round(float(np.median(ts)), 4), q1_ms=round(float(q1), 4), q3_ms=round(float(q3), 4), min_ms=round(float(ts.min()), 4),
                reps=int(ts.size))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="prod")
    ap.add_argument("--layers", type=int, default=1)
    ap.add_argument("--Q", type=int, default=3072)
    ap.add_argument("--n", default="1,4,8,16")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="timed calls per arm and block")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import recommendersystem_amd as ra
    from recommendersystem_amd import search, workload
    rng = np.random.default_rng(0)
    cfg = workload.make_config(a.shape, num_layers=a.layers)
    cfg["forward"] = "inference"
    cfg["finetune"] = False
    V = (cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"])
    D = cfg["embed_dim"]
    model = ra.RecommenderModel(cfg, dtype=a.dtype, max_rows=4)
    model.init_weights(7)
    model.random_pretrained_embeddings(8)
    W = (rng.standard_normal((a.Q, D), dtype=np.float32) * 1.5 / np.sqrt(a.Q)).astype(np.float32)
    results = []
    for m in (1, 0):
        s = search.SearchModel(search.training_config({m: V[m]}, batch_size=64, embed_dim=D, query_dim=a.Q), m, model, dtype=a.dtype, max_batch=64)
        s.param_set("encoder.weight", W)
        s.param_set("logit_scale", 1.0)
        for n in [int(x) for x in a.n.split(",")]:
            x = rng.standard_normal((n, a.Q), dtype=np.float32)
            group = np.zeros(n, np.int32)
            batch = {"queries": x, "matchedids": np.zeros(n, np.int64), "weight": np.ones(n)}
            arms = {"text_rows_setter": lambda: model.query_texts_set(s, m, x, group),
                    "gemm_scores_eval": lambda: s.forward_backward(batch, evaluate=True),
                    "search_topk_k1": lambda: s.topk(x, 1)}
            t = {k: [] for k in arms}
            for b in range(a.blocks):
                for k, fn in arms.items():
                    t[k] += timed(fn, 3 if b == 0 else 1, a.reps)
            model.query_texts_set(s, m, x[:0], [])                    # leave nothing pending
            res = dict(V_m=V[m], D=D, Q=a.Q, dtype=a.dtype, n=n, table_MB=round(V[m] * D * (2 if a.dtype == "bf16" else 4) / 1e6, 1),
                       **{k: stats(v) for k, v in t.items()})
            res["setter_over_gemm_scores"] = round(float(np.median(t["text_rows_setter"]) / np.median(t["gemm_scores_eval"])), 3)
            results.append(res)
            print(json.dumps(res), flush=True)
        s.close()
    model.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
