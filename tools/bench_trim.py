"""Inference on trimmed rows: the serving calls with `trim` off and on, alternating in one process on one model --
bf16, a four-adapter bank, max_rows 4, S = 1024, shapes cfg3 and prod (tools/bench_render.py's set-up).  Per shape and per history
length (30, 100, 300 and 1023 events; 1023 + the query token fill the row, so there `trim` on is the ordinary upload): a one-user
serve.predict retrieval, a one-user serve.render_users with full_history off and on, and case (c) of bench_render.py (8 states, 15
users).  Wall time per call (host clock around the synchronous call), warm, --reps repeats in three alternating blocks; median,
quartiles and extremes.  Beside each time the tokens the call's trunk forwards ran over ("forward.tokens" for predict; the sum of
rows * 2 * row_len over "forward_rows" for the pipelines), so that the time ratio reads against the token ratio.  `same_pages` (and
`same_values` for predict) are reported, not asserted: near-tied candidates reorder with the GEMM route at cfg-3 bf16 size.

    python tools/bench_trim.py --out profiles/trim_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_render import DIM, make_state, sparse_csc, stats, timed  # noqa: E402


def build(shape, seq, rng):
    import recommendersystem_amd as ra
    from recommendersystem_amd import serve, workload
    cfg = workload.make_config(shape)
    cfg["max_sequence_length"] = seq
    cfg["forward"] = "inference"
    cfg["finetune"] = False
    V = (cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"])
    model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=4)
    model.init_weights(7)
    model.random_pretrained_embeddings(8)
    model.adapter_slots = {}
    for slot, key in enumerate(("0.retrieval", "0.ranking", "1.retrieval", "1.ranking")):
        model.load_adapter(slot, {n: (0.02 * rng.standard_normal(s)).astype(np.float32) for n, s in model.adapter_names()})
        model.adapter_slots[key] = slot
    rel = {}
    for m in (0, 1):
        rel[f"{m}.dependencies"] = sparse_csc(rng, V[m], V[m], 0.05)
        rel[f"{m}.recaps"] = sparse_csc(rng, V[m], V[m], 0.02)
        rel[f"{m}.adaptations"] = sparse_csc(rng, V[m], V[1 - m], 0.05)
    sim = {f"embeddings.{m}": (rng.standard_normal((DIM, V[m])) / np.sqrt(DIM)).astype(np.float32) for m in (0, 1)}
    serve.load_retrieval_tables(model, rel, sim)
    serve.load_ranking_tables(model, {f"{m}.related": sparse_csc(rng, V[m], V[m], 3.0) for m in (0, 1)})
    registry = {f"{m}.rating.coefs": np.array([0.3, 0.8]) for m in (0, 1)}
    registry.update({f"{m}.rating_mean": 4.0 for m in (0, 1)})
    return model, V, registry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg3,prod")
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--events", default="30,100,300,1023")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from recommendersystem_amd import serve
    pag = {"offset": 0, "limit": 10}
    results = []
    for shape in a.shapes.split(","):
        rng = np.random.default_rng(1)
        model, V, registry = build(shape, a.seq, rng)
        pipeline_tokens = lambda: int(sum(r * 2 * rl for _, r, rl in model.render_kept("forward_rows").reshape(-1, 3).tolist()))
        for events in [int(x) for x in a.events.split(",")]:
            one = [make_state(rng, V, 0, 1, events)]
            many = [make_state(rng, V, g % 2, 1 + g % 3, events) for g in range(8)]
            user = one[0]["users"][0]["user"]
            calls = {
                "predict_retrieval_1_user": (lambda trim: serve.predict(model, [user], "retrieval", 0, trim=trim), lambda: model.forward_tokens),
                "render_users_1_user": (lambda trim: serve.render_users(model, one, pag, registry, trim=trim), pipeline_tokens),
                "render_users_full_1_user": (lambda trim: serve.render_users(model, one, pag, registry, full_history=True, trim=trim), pipeline_tokens),
                "render_users_c_8_states": (lambda trim: serve.render_users(model, many, pag, registry, trim=trim), pipeline_tokens),
            }
            for name, (fn, tokens) in calls.items():
                out, tok = {}, {}
                for trim in (False, True):
                    out[trim] = fn(trim); tok[trim] = tokens()
                if name.startswith("predict"):
                    same = bool(np.array_equal(out[False][0]["0.retrieval"], out[True][0]["0.retrieval"]))
                else:
                    same = bool(all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(out[False], out[True])))
                t = {False: [], True: []}
                blocks = 3
                for b in range(blocks):                                   # alternating blocks: off, on, off, on, ...
                    for trim in (False, True):
                        t[trim] += timed(lambda: fn(trim), a.warmup if b == 0 else 1, a.reps // blocks)
                off, on = stats(t[False]), stats(t[True])
                res = dict(call=name, shape=shape, S=a.seq, events=events, same_pages=same, trim_off=dict(off, forward_tokens=tok[False]),
                           trim_on=dict(on, forward_tokens=tok[True]), time_ratio_on_over_off=round(on["median_ms"] / off["median_ms"], 3),
                           token_ratio_on_over_off=round(tok[True] / tok[False], 3),
                           on_inside_off_spread=bool(off["min_ms"] <= on["median_ms"] <= off["max_ms"]),
                           on_slower_than_off_spread=bool(on["median_ms"] > off["max_ms"]))
                results.append(res)
                print(json.dumps(res), flush=True)
        model.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
