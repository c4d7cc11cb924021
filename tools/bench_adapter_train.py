"""Training through the adapter bank at the cfg-3 model size, bf16: (a) one joint micro-step of 4 x 16 rows plus its
optimizer step on one base model against (b) the four finetune = 1 models' 16-row micro-steps plus their optimizer steps, summed;
alternating in one process, medians of --calls calls after a warm-up, taken twice; and the device memory of both set-ups
(hipMemGetInfo before / after creation).

    python tools/bench_adapter_train.py [--config cfg3] [--calls 20] [--out profiles/adapter_train_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="a few joint steps only (run under rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
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
