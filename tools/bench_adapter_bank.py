"""Adapter bank at the cfg-3 model size, bf16: device memory of one base model + four adapter slots against four
finetune = 1 models (hipMemGetInfo before / after creation), time per request batch of the bank call against the finetune model's
rsys_infer_select on the same batch (1, 4, 16 users; retrieval and ranking; median of --calls calls after a warm-up), and a mixed
batch of two users of two media in one `serve.predict_mixed` call against two `serve.predict` calls.

    python tools/bench_adapter_bank.py [--config cfg3] [--calls 30] [--out profiles/adapter_bank_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_adapter_bank.py --trace     (a few bank calls only, for the kernel times)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recommendersystem_amd as ra  # noqa: E402
from recommendersystem_amd import serve, workload  # noqa: E402


def free_bytes():
    ra.lib()   # (loads the HIP runtime)
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def adapter(model, seed):
    rng = np.random.default_rng(seed)
    return {n: (rng.standard_normal(s) / np.sqrt(s[-1])).astype(np.float32) for n, s in model.adapter_names()}


def median_ms(fn, calls, warmup=5):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()                          # (every inference call ends in a device synchronise and the output copy)
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def user(rng, n_events, cands, n_items):
    items, ts = [], 1.2e9
    for _ in range(n_events):
        ts += float(rng.integers(10, 10 ** 6))
        items.append({"medium": int(rng.integers(0, 2)), "matchedid": int(rng.integers(1, n_items)), "history_max_ts": ts,
                      "status": int(rng.integers(0, 9)), "rating": float(rng.integers(0, 11)), "progress": float(rng.random()),
                      "history_status": -1, "history_rating": -1.0})
    return {"user": {"gender": None, "source": 2}, "items": items, "timestamp": ts + 60.0, "ranking_items": list(cands)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="a few bank calls only (run under rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    cfg = workload.make_config(a.config)
    cfg["forward"] = "inference"
    S, D = cfg["max_sequence_length"], cfg["embed_dim"]
    ft_cfg = dict(cfg, finetune=True, finetune_metric="rating", lora_dropout=0.0)
    rows_max = 16
    res = {"config": a.config, "dtype": "bf16", "max_rows": rows_max, "calls": a.calls}

    def batch(rows):
        d = workload.make_batch(cfg, rows, 5 + rows, mu=4.6, sigma=1.0)
        d["rope_input_pos"] = np.tile(np.arange(S, dtype=np.int32), rows)
        return d

    def tokens(rows, task):   # what a server reads (embed.py:147-161): one token per user, or S / 2 candidates' action tokens per user
        return np.concatenate([r * 2 * S + (np.array([2 * (S - 1)]) if task == "retrieval" else 2 * (S // 2 + np.arange(S // 2)) + 1)
                               for r in range(rows)])

    if a.trace:
        bank = ra.RecommenderModel(cfg, device=0, dtype="bf16", max_rows=rows_max)
        bank.init_weights(0x1217); bank.random_pretrained_embeddings(0x3E7A)
        for s in range(4):
            bank.load_adapter(s, adapter(bank, 100 + s))
        for rows in (1, 16):
            d = batch(rows)
            slots = [r % 4 for r in range(rows)]
            for _ in range(6):
                bank.inference_select(d, "retrieval", tokens(rows, "retrieval"), adapters=slots)
        bank.close()
        return

    # ---- device memory: four finetune = 1 models against one base model + four slots
    f0 = free_bytes()
    fts = []
    for s in range(4):
        m = ra.RecommenderModel(ft_cfg, device=0, dtype="bf16", max_rows=rows_max)
        m.init_weights(0x1217); m.random_pretrained_embeddings(0x3E7A)
        fts.append(m)
    f1 = free_bytes()
    for m in fts[1:]:
        m.close()
    ft = fts[0]
    f2 = free_bytes()
    bank = ra.RecommenderModel(cfg, device=0, dtype="bf16", max_rows=rows_max)
    bank.init_weights(0x1217); bank.random_pretrained_embeddings(0x3E7A)
    ads = [adapter(bank, 100 + s) for s in range(4)]
    for s in range(4):
        bank.load_adapter(s, ads[s])
    bank.inference_select(batch(rows_max), "retrieval", tokens(rows_max, "retrieval"), adapters=[0] * rows_max)   # (the rank-16 buffer is allocated on first use)
    f3 = free_bytes()
    res["memory"] = {"four_finetune_models_bytes": f0 - f1, "base_plus_four_slots_bytes": f2 - f3, "ratio": (f2 - f3) / max(1, f0 - f1)}
    print("memory", json.dumps(res["memory"]), flush=True)
    for k, v in ads[0].items():
        ft.set_parameter(k, v)

    # ---- time per request batch: the bank call against the finetune model's rsys_infer_select, alternating
    res["latency_ms"] = []
    for rows in (1, 4, 16):
        d = batch(rows)
        for task in ("retrieval", "ranking"):
            idx = tokens(rows, task)
            slots = [r % 4 for r in range(rows)]
            old = median_ms(lambda: ft.inference_select(d, task, idx), a.calls)
            new = median_ms(lambda: bank.inference_select(d, task, idx, adapters=slots), a.calls)
            old2 = median_ms(lambda: ft.inference_select(d, task, idx), a.calls)
            new2 = median_ms(lambda: bank.inference_select(d, task, idx, adapters=slots), a.calls)
            base = median_ms(lambda: bank.inference_select(d, task, idx), a.calls)
            row = {"rows": rows, "task": task, "finetune_model_median": [old[0], old2[0]], "bank_median": [new[0], new2[0]],
                   "finetune_model_min": min(old[1], old2[1]), "bank_min": min(new[1], new2[1]), "base_model_median": base[0],
                   "bank_over_finetune": (new[0] + new2[0]) / (old[0] + old2[0])}
            res["latency_ms"].append(row)
            print("latency", json.dumps(row), flush=True)
    ft.close()

    # ---- two users of two media: one predict_mixed call against two predict calls
    bank.adapter_slots = {"0.retrieval": 0, "0.ranking": 1, "1.retrieval": 2, "1.ranking": 3}
    rng = np.random.default_rng(3)
    n_items = min(cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"])
    res["mixed_ms"] = []
    for task in ("retrieval", "ranking"):
        us = [user(rng, 200, rng.integers(1, n_items, 64).tolist(), n_items) for _ in range(2)]
        two = median_ms(lambda: (serve.predict(bank, [us[0]], task, 0), serve.predict(bank, [us[1]], task, 1)), a.calls)
        one = median_ms(lambda: serve.predict_mixed(bank, [(us[0], 0), (us[1], 1)], task), a.calls)
        row = {"task": task, "two_predict_calls_median": two[0], "one_predict_mixed_call_median": one[0]}
        res["mixed_ms"].append(row)
        print("mixed", json.dumps(row), flush=True)
    bank.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
