"""Times the search model (rsys_search_*) at the reference shape on synthetic data: one training step (forward +
soft-max loss + backward + AdamW), one forward-only eval batch, the export and the top-k serving call, for each V_m given.  Prints one
JSON line (median wall ms of synchronous calls after a warm-up; the calls include the host-side checks and the upload of the batch)
and writes it to profiles/search_bench.json (--out FILE, '' = nowhere).  --host 1 also times the numpy path (fp32 BLAS on the cores the process may use) for the
export and the top-k.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats`.

  python tools/bench_search.py [--B 1024 --D 2048 --Q 3072 --V 80000,120000 --dtype bf16 --reps 5 --k 1024 --host 0 --out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FLOPS = 2.5e15      # dense bf16 MFMA peak the project's rooflines use
STREAM_BPS = 5.0e12      # the stream rate the project measures


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--D", type=int, default=2048)
    ap.add_argument("--Q", type=int, default=3072)
    ap.add_argument("--V", default="80000,120000")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--nq", default="1,16,256")
    ap.add_argument("--host", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "search_bench.json"),
                    help="where the JSON is written ('' = nowhere)")
    a = ap.parse_args()
    from recommendersystem_amd import search
    rng = np.random.default_rng(0)

    def timed(fn):
        fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), ts

    res = {"shape": vars(a), "cases": []}
    W = (rng.standard_normal((a.Q, a.D), dtype=np.float32) * 1.5 / np.sqrt(a.Q)).astype(np.float32)
    for V in [int(v) for v in a.V.split(",")]:
        feat = rng.standard_normal((V, a.D), dtype=np.float32) / np.float32(np.sqrt(a.D))
        cfg = search.training_config({0: V}, batch_size=a.B, embed_dim=a.D, query_dim=a.Q)
        m = search.SearchModel(cfg, 0, feat, dtype=a.dtype)
        m.param_set("encoder.weight", W)
        m.create_optimizer()
        batch = {"queries": rng.standard_normal((a.B, a.Q), dtype=np.float32), "matchedids": rng.integers(0, V, a.B),
                 "weight": np.sqrt(rng.integers(1, 100, a.B).astype(np.float64))}

        def step():
            m.zero_grad()
            m.forward_backward(batch)
            m.adamw_step(3e-4, 1.0)

        c = {"V_m": V}
        c["step_ms"], c["step_all_ms"] = timed(step)
        c["fwd_bwd_ms"], _ = timed(lambda: m.forward_backward(batch))
        c["eval_ms"], _ = timed(lambda: m.forward_backward(batch, evaluate=True))
        c["export_ms"], _ = timed(m.embed)
        for nq in [int(x) for x in a.nq.split(",")]:
            xq = batch["queries"][:nq]
            c[f"topk_nq{nq}_ms"], _ = timed(lambda: m.topk(xq, min(a.k, V)))
        # the roofline the step is judged against: two [B][D] x [D][V] products and two with x at the MFMA peak, and the passes over
        # the score slab (fp32 written and read twice, G written and read once in the operand dtype) at the stream rate
        flops = 2 * 2.0 * a.B * a.D * V + 2 * 2.0 * a.B * a.Q * a.D
        tsz = 2 if a.dtype == "bf16" else 4
        slab_bytes = a.B * V * (3 * 4 + 2 * tsz)
        c["step_tflop"] = flops / 1e12
        c["roofline_gemm_ms"] = flops / PEAK_FLOPS * 1e3
        c["roofline_slab_ms"] = slab_bytes / STREAM_BPS * 1e3
        if a.host:
            E32 = feat

            def host_export():
                return E32 @ W.T

            def host_topk(nq):
                z = (batch["queries"][:nq] @ W) @ E32.T * np.float32(np.e)
                z -= z.max(axis=1, keepdims=True)
                lp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
                return np.argsort(-lp, axis=1, kind="stable")[:, :a.k]

            c["host_numpy_export_ms"], _ = timed(host_export)
            for nq in [int(x) for x in a.nq.split(",")]:
                c[f"host_numpy_topk_nq{nq}_ms"], _ = timed(lambda: host_topk(nq))
            c["host_threads"] = os.environ.get("OMP_NUM_THREADS", "")
        res["cases"].append(c)
        m.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
