"""Times the item-similarity LambdaRank model (rsys_sim_*) at the reference shape on synthetic data: one training step
(forward + LambdaRank + backward + AdamW), one nDCG eval batch, the export of every id, and the hard-negative mining.  Prints one JSON
line (median wall ms of synchronous calls after warm-up).  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats`.

  python tools/bench_similarity.py [--nq 128 --n 2048 --F 2048 --E 1024 --V 80000 --dtype bf16 --reps 5 --mine 1024]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=128)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--F", type=int, default=2048)
    ap.add_argument("--E", type=int, default=1024)
    ap.add_argument("--V", type=int, default=80000)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mine", type=int, default=1024, help="sources per hard-negative mining call")
    a = ap.parse_args()
    from recommendersystem_amd import similarity as sim
    from recommendersystem_amd._lib import check, lib
    import ctypes as C
    rng = np.random.default_rng(0)
    feat = rng.standard_normal((a.V, a.F), dtype=np.float32)
    cfg = sim.training_config({0: a.V}, embed_dim=a.E, batch_size=a.nq, items_per_query=a.n)
    m = sim.LTRModel(cfg, 0, feat, dtype=a.dtype, dropout=0.1)
    m.param_set("encoder.1.weight", (rng.standard_normal((a.E, a.F), dtype=np.float32) / np.sqrt(a.F)))
    src = rng.integers(0, a.V, a.nq)
    npos = int(a.n * 0.9)
    rel = np.zeros((a.nq, a.n))
    rel[:, :npos] = rng.integers(1, 100, (a.nq, npos))
    batch = {"sourceid": np.repeat(src[:, None], a.n, 1), "targetid": rng.integers(0, a.V, (a.nq, a.n)), "relevance": rel,
             "weight": np.sqrt(rng.integers(1, 1000, (a.nq, 1)).astype(np.float64))}
    words = (a.V + 31) // 32
    bits = np.where(rng.random((a.V, words), dtype=np.float32) < 0.5, 1 << rng.integers(0, 31, (a.V, words)), 0).astype(np.int32)
    check(lib().rsys_sim_testmask_set(m.h, bits.ctypes.data_as(C.c_void_p)))
    del bits
    sources = rng.integers(0, a.V, a.mine)
    positives = [rng.integers(0, a.V, npos).tolist() for _ in range(a.mine)]

    def timed(fn):
        fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), ts

    def step():
        m.zero_grad()
        m.forward_backward(batch)
        m.adamw_step(3e-4, 1.0)
        m.step += 1

    res = {"shape": vars(a)}
    res["step_ms"], res["step_all_ms"] = timed(step)
    res["fwd_bwd_ms"], _ = timed(lambda: m.forward_backward(batch))
    res["eval_ndcg_ms"], _ = timed(lambda: m.ndcg(batch))
    res["export_ms"], _ = timed(lambda: m.embed_all(train_mode=False))
    res["export_train_mode_ms"], _ = timed(lambda: m.embed_all(train_mode=True))
    res["mine_ms"], _ = timed(lambda: m.hard_negatives("training", sources, positives, a.n))
    res["mine_us_per_source"] = res["mine_ms"] * 1e3 / a.mine
    P = 2 * a.nq * a.n
    res["gemm_tflop_per_step"] = 2 * 2.0 * P * a.F * a.E / 1e12
    res["pairs_per_step"] = a.nq * a.n * a.n
    print(json.dumps(res))


if __name__ == "__main__":
    main()
