"""Shared by the adapter-bank tests: synthetic users, adapters and finetune checkpoints (inputs only, no model arithmetic)."""
import numpy as np

ORDER = [(0, "watch"), (0, "rating"), (1, "watch"), (1, "rating")]      # Finetune/run.jl:9-13
SLOT_MAP = {"0.retrieval": 0, "0.ranking": 1, "1.retrieval": 2, "1.ranking": 3}


def make_user(rng, n_events, cands, n_items=25):
    items, ts = [], 1.2e9
    for _ in range(n_events):
        ts += float(rng.integers(10, 10 ** 6))
        items.append({"medium": int(rng.integers(0, 2)), "matchedid": int(rng.integers(1, n_items)), "history_max_ts": ts,
                      "status": int(rng.integers(0, 9)), "rating": float(rng.integers(0, 11)), "progress": float(rng.random()),
                      "history_status": -1, "history_rating": -1.0})
    return {"user": {"gender": None, "source": 2}, "items": items, "timestamp": ts + 60.0, "ranking_items": list(cands)}


def finetune_config(cfg):
    ft = dict(cfg)
    ft["vocab_sizes"] = dict(cfg["vocab_sizes"])
    ft.update(finetune=True, finetune_metric="rating", lora_dropout=0.0)
    return ft


def make_adapters(cfg, n, seed):
    """n LoRA adapter sets in oracle.synth's "test" style: A ~ N(0, 1 / D), B ~ N(0, 1 / 8) -- with xn of order one the update
    2 (xn A^T) B^T has about twice the standard deviation of the projection xn W^T (W ~ N(0, 1 / D)) it is added to."""
    from oracle import synth
    ft = finetune_config(cfg)
    return [{k: v for k, v in synth.make_params(ft, seed + i, "test").items() if "lora_" in k} for i in range(n)]


def finetune_blobs(cfg, P, adapters):
    """four finetune checkpoints in the `.npz` layout (train.checkpoint_model): the same trunk, one adapter each"""
    blobs = []
    for i, ad in enumerate(adapters):
        blob = {"model/" + k: v for k, v in P.items()}
        blob.update({"model/" + k: v for k, v in ad.items()})
        blob["epoch"] = np.array([i])
        blobs.append(blob)
    return blobs
