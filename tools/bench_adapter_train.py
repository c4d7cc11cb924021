"""Training through the adapter bank at the cfg-3 model size, bf16: (a) one joint micro-step of 4 x 16 rows plus its
optimizer step on one base model against (b) the four finetune = 1 models' 16-row micro-steps plus their optimizer steps, summed;
alternating in one process, medians of --calls calls after a warm-up, taken twice; and the device memory of both set-ups
(hipMemGetInfo before / after creation).

    python tools/bench_adapter_train.py [--config cfg3] [--calls 20] [--out profiles/adapter_train_bench.json]
    python tools/bench_adapter_train.py --pack [--out profiles/adapter_pack_train_bench.json]     (packed rows, DESIGN 4zc: see pack_bench)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_adapter_train.py --trace     (a few joint steps only)
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
from recommendersystem_amd import workload  # noqa: E402
from recommendersystem_amd.optim import AdamW, AdapterAdamW  # noqa: E402

METRICS = ("watch", "rating")
ROWS = 16


def free_bytes():
    ra.lib()   # (loads the HIP runtime)
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def adapter(model, seed):
    rng = np.random.default_rng(seed)
    return {n: (rng.standard_normal(s) / np.sqrt(s[-1])).astype(np.float32) for n, s in model.adapter_names()}


def median_ms(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()                          # (every step ends in the loss read-back and the norms' copy: both synchronise)
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def finetune_users(cfg, users, events, seed, task):
    """`users` finetune rows of task (medium, metric): `events` live columns cut from the synthetic stream as ONE user each, zeros
    behind, and one target -- the last event, an item of the task's medium -- as the reference's FinetuneDataset rows carry it"""
    S = cfg["max_sequence_length"]
    m, metric = task >> 1, METRICS[task & 1]
    d = {k: np.array(np.asarray(v).reshape(users, S)) for k, v in workload.make_batch(cfg, users, seed).items()}
    for k, v in d.items():
        v[:, events:] = 0
        if k.endswith(".weight"):
            v[:] = 0
    d["userid"][:, :events] = 1 + np.arange(users)[:, None]
    last = events - 1
    d["matchedid"][:, last] = 5 + (cfg["vocab_sizes"]["0_matchedid"] if m == 1 else 0)
    d["token_mask_ids"][:, last] = 1
    d[f"{m}.{metric}.weight"][:, last] = 1
    d[f"{m}.{metric}.label"][:, last] = 1 if metric == "watch" else 7
    d[f"{m}.{metric}.position"][:, last] = 5
    return {k: v.reshape(-1) for k, v in d.items()}


def pack_bench(a):
    """Packed against unpacked joint steps at the cfg-3 size, bf16: four slots x 16 users of `events` live events each.
    Arm (a): the unpacked joint step, one user per row (64 rows); arm (b): the packed step on the same users (train.pack_adapter_rows).
    Both models live in this process, the arms alternate (a b a b), every figure is the median of --calls steps after a warm-up, and
    every step ends in its loss read-back and the optimizer's norm copy (both synchronise).  events = S: 64 full-length users, the
    same rows in both arms -- what is left is the packed pass's dense last layer."""
    from recommendersystem_amd.train import pack_adapter_batch, pack_adapter_rows
    lines = []
    for S in (512, 1024):
        cfg = workload.make_config(a.config, max_sequence_length=S)
        cfg["forward"] = "train"
        banks = []
        for _ in range(2):
            bank = ra.RecommenderModel(cfg, device=0, dtype="bf16", max_rows=4 * ROWS)
            bank.init_weights(0x1217); bank.random_pretrained_embeddings(0x3E7A)
            for s in range(4):
                bank.load_adapter(s, adapter(bank, 100 + s))
            bank.enable_adapter_training(0.1)
            banks.append((bank, AdapterAdamW(bank, lr=2e-4, slots=range(4))))
        (flat_bank, flat_opt), (pack_bank, pack_opt) = banks
        for events in (30, 100, 300, S):
            subs = [(s, s, finetune_users(cfg, ROWS, events, 11 + s, s)) for s in range(4)]
            flat, row_slot, row_task = pack_adapter_batch(subs, S)
            packed, segs = pack_adapter_rows(subs, S, 4 * ROWS, cfg["mask_topk"])
            flat_bank.upload(flat); pack_bank.upload(packed)

            def step_a():
                flat_bank.forward_backward_adapters(None, row_slot, row_task)
                flat_opt.step({s: 1.0 for s in range(4)}, clip_max_norm=1.0)

            def step_b():
                pack_bank.forward_backward_adapters_packed(None, segs)
                pack_opt.step({s: 1.0 for s in range(4)}, clip_max_norm=1.0)

            if a.trace:
                for _ in range(5):
                    step_b()
                continue
            ta, tb = median_ms(step_a, a.calls), median_ms(step_b, a.calls)
            ta2, tb2 = median_ms(step_a, a.calls), median_ms(step_b, a.calls)
            rows_b = packed["userid"].size // S
            line = {"config": a.config, "dtype": "bf16", "S": S, "events": events, "users": 4 * ROWS, "calls": a.calls,
                    "unpacked": {"rows": 4 * ROWS, "tokens": 4 * ROWS * 2 * S, "median_ms": [ta[0], ta2[0]], "min_ms": min(ta[1], ta2[1])},
                    "packed": {"rows": rows_b, "tokens": rows_b * 2 * S, "median_ms": [tb[0], tb2[0]], "min_ms": min(tb[1], tb2[1])},
                    "packed_over_unpacked_time": (tb[0] + tb2[0]) / (ta[0] + ta2[0]), "packed_over_unpacked_tokens": rows_b / (4.0 * ROWS),
                    "packed_median_below_unpacked_min": max(tb[0], tb2[0]) < min(ta[1], ta2[1])}
            lines.append(line)
            print("pack", json.dumps(line), flush=True)
        for bank, _ in banks:
            bank.close()
    if a.out and not a.trace:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="a few joint steps only (run under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--pack", action="store_true", help="packed against unpacked joint steps at S = 512 and 1024 (DESIGN 4zc)")
    a = ap.parse_args()
    if a.pack:
        return pack_bench(a)
    cfg = workload.make_config(a.config)
    cfg["forward"] = "train"
    S = cfg["max_sequence_length"]
    res = {"config": a.config, "dtype": "bf16", "rows_per_adapter": ROWS, "calls": a.calls}
    subs = [workload.make_batch(cfg, ROWS, 11 + s) for s in range(4)]
    joint_batch = {k: np.concatenate([np.asarray(d[k]).reshape(-1) for d in subs]) for k in subs[0]}
    row_slot = np.repeat(np.arange(4, dtype=np.int32), ROWS)

    def make_bank():
        bank = ra.RecommenderModel(cfg, device=0, dtype="bf16", max_rows=4 * ROWS)
        bank.init_weights(0x1217); bank.random_pretrained_embeddings(0x3E7A)
        for s in range(4):
            bank.load_adapter(s, adapter(bank, 100 + s))
        bank.enable_adapter_training(0.1)
        bank.upload(joint_batch)
        return bank, AdapterAdamW(bank, lr=2e-4, slots=range(4))

    def joint_step(bank, opt):
        bank.forward_backward_adapters(None, row_slot, row_slot)
        opt.step({s: 1.0 for s in range(4)}, clip_max_norm=1.0)

    if a.trace:
        bank, opt = make_bank()
        for _ in range(5):
            joint_step(bank, opt)
        bank.close()
        return

    f0 = free_bytes()
    fts = []
    for s in range(4):
        m = ra.RecommenderModel(dict(cfg, finetune=True, finetune_metric=METRICS[s & 1]), device=0, dtype="bf16", max_rows=ROWS)
        m.init_weights(0x1217); m.random_pretrained_embeddings(0x3E7A)
        m.set_loss_weights([1.0 if i == s else 0.0 for i in range(4)], 1)
        m.upload(subs[s])
        fts.append((m, AdamW(m, lr=2e-4)))
    f1 = free_bytes()
    bank, opt = make_bank()
    joint_step(bank, opt)
    f2 = free_bytes()
    res["memory"] = {"four_finetune_models_bytes": f0 - f1, "base_model_with_bank_training_bytes": f1 - f2, "ratio": (f1 - f2) / max(1, f0 - f1)}
    print("memory", json.dumps(res["memory"]), flush=True)

    def four_steps():
        for m, o in fts:
            m.forward_resident(False)
            m.losses(False)
            o.step(clip_max_norm=1.0)

    old = median_ms(four_steps, a.calls); new = median_ms(lambda: joint_step(bank, opt), a.calls)
    old2 = median_ms(four_steps, a.calls); new2 = median_ms(lambda: joint_step(bank, opt), a.calls)
    res["step_ms"] = {"four_finetune_models_median": [old[0], old2[0]], "joint_median": [new[0], new2[0]],
                      "four_finetune_models_min": min(old[1], old2[1]), "joint_min": min(new[1], new2[1]),
                      "four_finetune_models_spread": abs(old[0] - old2[0]), "joint_spread": abs(new[0] - new2[0]),
                      "joint_over_four": (new[0] + new2[0]) / (old[0] + old2[0])}
    print("step", json.dumps(res["step_ms"]), flush=True)
    for m, _ in fts:
        m.close()
    bank.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
