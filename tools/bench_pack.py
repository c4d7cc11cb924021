"""Several users per serving row: the serving calls with `trim=True` (one user per row) against `pack=True`, alternating in
one process on one model -- bf16, a four-adapter bank, max_rows 4, S = 1024, shapes cfg3 and prod (tools/bench_trim.py's set-up).  Per
shape: serve.predict retrieval for 4, 16 and 64 users of 30, 100 and 300 events (the `trim` arm serves them as a server does today, in
calls of max_rows users; the `pack` arm in one call), and case (c) of bench_render.py (8 states, 15 users) through serve.render_users.
Wall time per request (host clock around the synchronous calls, so the host's batch assembly is inside it for both arms), warm, --reps
repeats in three alternating blocks; median, quartiles and extremes.  Beside each time the trunk forwards the request took and the
tokens they ran over.  `same_values` / `same_pages` are reported, not asserted (near-tied candidates reorder with the GEMM
route at cfg-3 bf16 size).

    python tools/bench_pack.py --out profiles/pack_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_render import make_state, stats, timed  # noqa: E402
from bench_trim import build  # noqa: E402


class Forwards:
    """forwards and tokens of the `inference_select` calls made on `model` while it is open"""

    def __init__(self, model):
        self.model, self.n, self.tokens = model, 0, 0

    def __enter__(self):
        inner = self.model.inference_select

        def counted(*a, **kw):
            out = inner(*a, **kw)
            self.n += 1; self.tokens += self.model.forward_tokens
            return out
        self.model.inference_select = counted
        return self

    def __exit__(self, *exc):
        del self.model.inference_select


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg3,prod")
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--users", default="4,16,64")
    ap.add_argument("--events", default="30,100,300")
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
        R = model.max_rows

        def predict_arm(users, pack):
            if pack:
                return serve.predict(model, users, "retrieval", 0, pack=True)
            out = []
            for u0 in range(0, len(users), R):
                out += serve.predict(model, users[u0:u0 + R], "retrieval", 0, trim=True)
            return out

        def pipeline_counts():
            fr = model.render_kept("forward_rows").reshape(-1, 3)
            return int(len(fr)), int((2 * fr[:, 1] * fr[:, 2]).sum()), int((fr[:, 0] == 0).sum())

        cases = []
        for events in [int(x) for x in a.events.split(",")]:
            for n_users in [int(x) for x in a.users.split(",")]:
                users = [make_state(rng, V, 0, 1, events)["users"][0]["user"] for _ in range(n_users)]
                cases.append((f"predict_retrieval_{n_users}_users", events, (lambda pack, users=users: predict_arm(users, pack)), True))
            many = [make_state(rng, V, g % 2, 1 + g % 3, events) for g in range(8)]
            cases.append(("render_users_c_8_states", events,
                          (lambda pack, many=many: serve.render_users(model, many, pag, registry, trim=True, pack=pack)), False))
        for name, events, fn, is_predict in cases:
            out, count = {}, {}
            for pack in (False, True):
                if is_predict:
                    with Forwards(model) as f:
                        out[pack] = fn(pack)
                    count[pack] = dict(forwards=f.n, forward_tokens=f.tokens)
                else:
                    out[pack] = fn(pack)
                    n, tok, n0 = pipeline_counts()
                    count[pack] = dict(forwards=n, forward_tokens=tok, retrieval_forwards=n0)
            if is_predict:
                same = bool(all(np.array_equal(x["0.retrieval"], y["0.retrieval"]) for x, y in zip(out[False], out[True])))
            else:
                same = bool(all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(out[False], out[True])))
            t = {False: [], True: []}
            blocks = 3
            for b in range(blocks):                                       # alternating blocks: trim, pack, trim, pack, ...
                for pack in (False, True):
                    t[pack] += timed(lambda: fn(pack), a.warmup if b == 0 else 1, a.reps // blocks)
            trim, pk = stats(t[False]), stats(t[True])
            res = dict(call=name, shape=shape, S=a.seq, events=events, **{"same_values" if is_predict else "same_pages": same},
                       trim=dict(trim, **count[False]), pack=dict(pk, **count[True]),
                       time_ratio_pack_over_trim=round(pk["median_ms"] / trim["median_ms"], 3),
                       token_ratio_pack_over_trim=round(count[True]["forward_tokens"] / count[False]["forward_tokens"], 3),
                       pack_inside_trim_spread=bool(trim["min_ms"] <= pk["median_ms"] <= trim["max_ms"]),
                       pack_slower_than_trim_spread=bool(pk["median_ms"] > trim["max_ms"]))
            results.append(res)
            print(json.dumps(res), flush=True)
        model.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
