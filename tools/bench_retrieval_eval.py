"""Finetune evaluation on the device (rsys_retrieve_target_rank: the target rank and log-probability of Finetune/regress.jl's
`retrieval_metrics` / `regress_retrieval`) against rsys_retrieve_topk at k = 1024 for the same users and against the host path it replaces
(numpy `compute_retrieval`, a soft-max over the medium's whole item table, plus a full sort per user).

bf16 models at the cfg-3 (D = 512) and production (D = 2048) widths with V_0 = 120 000, medium 0, 256 / 4096 / 16 384 users (calls of
more than 4096 users are split by RecommenderModel.retrieve_target_rank), exclusions of item 0 plus 30 ids per user.  Wall times,
median of --reps after --warmup.  The host path is timed for two users and scaled.  The per-kernel split comes from a
`rocprofv3 --kernel-trace --stats` run of this script.

    python tools/bench_retrieval_eval.py --out profiles/retrieval_eval_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V0, V1 = 120000, 40000


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
    ap.add_argument("--users", default="256,4096,16384")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import recommendersystem_amd as ra
    from recommendersystem_amd import serve, workload
    rng = np.random.default_rng(1)
    m = 0
    results = []
    for shape in a.shapes.split(","):
        cfg = workload.make_config(shape)
        cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"] = V0, V1
        model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=1)
        model.init_weights(7)
        model.random_pretrained_embeddings(8)
        D = cfg["embed_dim"]
        F = model.item_embeddings()[:V0]
        reg = {"0.watch.weight": F}
        for n in (int(x) for x in a.users.split(",")):
            q = (rng.standard_normal((n, D)) / np.sqrt(D)).astype(np.float32)
            t = rng.integers(1, V0, n).astype(np.int32)
            excl = [np.concatenate([[0], rng.integers(0, V0, 30)]) for _ in range(n)]
            t_eval = timed(lambda: model.retrieve_target_rank(q, m, t, exclude=excl), a.warmup, a.reps)
            t_plain = timed(lambda: model.retrieve_target_rank(q, m, t), a.warmup, a.reps)

            def topk():
                for s in range(0, n, 4096):
                    model.retrieve_topk(q[s:s + 4096], m, 1024, exclude=excl[s:s + 4096])
            t_topk = timed(topk, 1, max(1, a.reps // 2))

            def host_two():
                for j in range(2):
                    p = serve.compute_retrieval(reg, m, {"0.retrieval": q[j]})
                    lp = np.log(p.astype(np.float64))
                    lp[excl[j]] = -np.inf
                    np.argsort(-lp, kind="stable")
            t_host2 = timed(host_two, 0, 1)
            res = dict(shape=shape, D=D, V_m=V0, users=n, calls=(n + 4095) // 4096, device_ms=round(t_eval, 3),
                       device_no_exclusions_ms=round(t_plain, 3), device_us_per_user=round(1e3 * t_eval / n, 3),
                       topk_1024_ms=round(t_topk, 3), host_path_ms=round(t_host2 * n / 2, 1), host_path_two_users_ms=round(t_host2, 1))
            results.append(res)
            print(json.dumps(res), flush=True)
        model.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
