"""The serving compact top: every serving call with `compact_top=False` against `compact_top=True`, each on top of the
best existing layout, alternating in blocks in one process on one model -- bf16, a four-adapter bank, max_rows 4, S = 1024, shapes cfg3
and prod (tools/bench_trim.py's set-up; tools/bench_rank_pack.py's method).  Per shape:
  * serve.predict (retrieval) for 1 user (trim=True) and 64 users (pack=True) of 30 / 300 / 1000 events;
  * serve.predict_ranking_full(pack=True) for 16 and 64 users of 30 / 300 events with 20 candidates, and 8 users of 300 events with S + 5;
  * serve.render_users(full_history=True, pack=True, pack_ranking=True) for tools/bench_render.py's cases a / b / c at 300 / 1000 events;
  * on the first shape, one sweep of n_sel across the attention rule's boundary (4 full rows: rows * ceil(T / 64) = 128 selected tokens):
    at each n_sel the dense pass, the compact tail behind the dense attention and a row gather (switch value 2) and the compact tail behind
    attn_sel_kernel (switch value 3), so that the rule can be read off the table.
Wall time per request (host clock around the synchronous call: the host's batch assembly is inside it for every arm), warm, --reps repeats
in three alternating blocks; median, quartiles and extremes.  Beside each time the trunk forwards the request took, the tokens they ran
over and what their last layers did ("infer.top" per forward).  Every row is reported, losers included; nothing is asserted.

    python tools/bench_compact_top.py --out profiles/compact_top_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_render import make_state, make_user, stats, timed  # noqa: E402
from bench_trim import build  # noqa: E402

CALLS = ("inference_select", "rank_cache_store", "rank_cache_candidates", "rank_cache_store_packed", "rank_cache_candidates_packed")


class Forwards:
    """forwards, tokens and last-layer modes of the trunk calls made on `model` while it is open"""

    def __init__(self, model):
        self.model, self.n, self.tokens, self.tops = model, 0, 0, []

    def __enter__(self):
        for name in CALLS:
            def counted(*a, _inner=getattr(self.model, name), **kw):
                out = _inner(*a, **kw)
                self.n += 1; self.tokens += self.model.forward_tokens
                self.tops.append(int(self.model.debug_get("infer.top", 0)[0]))
                return out
            setattr(self.model, name, counted)
        return self

    def __exit__(self, *exc):
        for name in CALLS:
            delattr(self.model, name)

    def counts(self):
        return dict(forwards=self.n, forward_tokens=self.tokens, infer_top={str(m): self.tops.count(m) for m in sorted(set(self.tops))})


def ab(fn, warmup, reps, arms=(False, True), blocks=3):
    """alternating blocks: arm 0, arm 1, ..., arm 0, ...; returns {arm: stats}"""
    t = {arm: [] for arm in arms}
    for b in range(blocks):
        for arm in arms:
            t[arm] += timed(lambda: fn(arm), warmup if b == 0 else 1, max(1, reps // blocks))
    return {arm: stats(ts) for arm, ts in t.items()}


def worst_difference(x, y):
    d = 0.0
    for p, q in zip(x, y):
        for k in p:
            a, b = np.asarray(p[k], np.float64), np.asarray(q[k], np.float64)
            if a.size:
                d = max(d, float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg3,prod")
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from recommendersystem_amd import serve
    results = []

    def report(res):
        results.append(res)
        print(json.dumps(res), flush=True)
        if a.out:                                                         # (rewritten after every row: a run cut short keeps what it measured)
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)

    for si, shape in enumerate(a.shapes.split(",")):
        rng = np.random.default_rng(1)
        model, V, registry = build(shape, a.seq, rng)
        S = a.seq

        def measure(call, fn, **extra):
            out, count = {}, {}
            for on in (False, True):
                with Forwards(model) as f:
                    out[on] = fn(on)
                count[on] = f.counts()
            t = ab(fn, a.warmup, a.reps)
            report(dict(call=call, shape=shape, S=S, max_rel_difference=worst_difference(out[True], out[False]), off=dict(t[False], **count[False]),
                        on=dict(t[True], **count[True]), time_ratio_on_over_off=round(t[True]["median_ms"] / t[False]["median_ms"], 3),
                        on_slower_than_off_spread=bool(t[True]["median_ms"] > t[False]["max_ms"]), **extra))

        for events in (30, 300, 1000):
            one = [make_user(rng, V, events)["user"]]
            many = [make_user(rng, V, events)["user"] for _ in range(64)]
            measure("predict_retrieval_1_user_trim", lambda on: serve.predict(model, one, "retrieval", 0, trim=True, compact_top=on), events=events)
            measure("predict_retrieval_64_users_pack", lambda on: serve.predict(model, many, "retrieval", 0, pack=True, compact_top=on), events=events)

        def users_of(n, events, cands):
            return [dict(make_user(rng, V, events)["user"], ranking_items=[int(c) for c in rng.integers(1, V[0], size=cands)]) for _ in range(n)]

        cases = [(f"{n}_users_20_candidates", ev, users_of(n, ev, 20)) for ev in (30, 300) for n in (16, 64)]
        cases.append((f"8_users_{S + 5}_candidates", 300, users_of(8, 300, S + 5)))
        for name, events, users in cases:
            measure("predict_ranking_full_pack_" + name, lambda on: serve.predict_ranking_full(model, users, 0, pack=True, compact_top=on), events=events)

        pag = {"offset": 0, "limit": 10}
        model.rank_cache_reserve(4 * model.max_rows)
        for events in (300, 1000):
            for name, states in (("a_1_user", [make_state(rng, V, 0, 1, events)]), ("b_3_users", [make_state(rng, V, 0, 3, events)]),
                                 ("c_8_states", [make_state(rng, V, g % 2, 1 + g % 3, events) for g in range(8)])):
                fn = lambda on: serve.render_users(model, states, pag, registry, full_history=True, pack=True, pack_ranking=True, compact_top=on)
                out, count = {}, {}
                for on in (False, True):
                    out[on] = fn(on)
                    fr = model.render_kept("forward_rows").reshape(-1, 3)
                    ft = model.render_kept("forward_top").reshape(-1, 2)
                    count[on] = dict(forwards=int(len(fr)), forward_tokens=int((2 * fr[:, 1] * fr[:, 2]).sum()),
                                     infer_top={str(m): int((ft[:, 0] == m).sum()) for m in sorted(set(ft[:, 0].tolist()))}, top_rows=int(ft[:, 1].sum()))
                same = bool(all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(out[False], out[True])))
                t = ab(fn, a.warmup, a.reps)
                report(dict(call="render_users_full_pack_" + name, shape=shape, S=S, events=events, same_pages=same, off=dict(t[False], **count[False]),
                            on=dict(t[True], **count[True]), time_ratio_on_over_off=round(t[True]["median_ms"] / t[False]["median_ms"], 3),
                            on_slower_than_off_spread=bool(t[True]["median_ms"] > t[False]["max_ms"])))

        if si == 0:
            # the attention rule's boundary: 4 full rows, n_sel tokens spread evenly; arms 0 dense, 2 gather behind the dense attention, 3 attn_sel_kernel
            users = [make_user(rng, V, S - 1)["user"] for _ in range(model.max_rows)]
            d = serve.build_batch(users, "retrieval", 0, V[0], *serve._request_lengths(model, "retrieval", None, None))
            NT = model.max_rows * 2 * S
            boundary = model.max_rows * (2 * S // 64)
            for n_sel in (4, 32, boundary // 2, boundary, 2 * boundary, 4 * boundary, 8 * boundary):
                index = [int(x) for x in np.linspace(0, NT - 1, n_sel).astype(np.int64)]

                def run(arm):
                    model.serving_compact_top(arm)
                    try:
                        return model.inference_select(d, "retrieval", index)
                    finally:
                        model.serving_compact_top(False)

                tops = {}
                for arm in (0, 2, 3):
                    run(arm)
                    tops[arm] = int(model.debug_get("infer.top", 0)[0])
                t = ab(run, a.warmup, a.reps, arms=(0, 2, 3))
                report(dict(call="n_sel_sweep_retrieval_4_full_rows", shape=shape, S=S, n_sel=n_sel, rule_boundary=boundary, rule_picks="attn_sel" if n_sel <= boundary else "gather",
                            dense=dict(t[0], infer_top=tops[0]), gather=dict(t[2], infer_top=tops[2]), attn_sel=dict(t[3], infer_top=tops[3]),
                            time_ratio_attn_sel_over_gather=round(t[3]["median_ms"] / t[2]["median_ms"], 3)))
        model.close()


if __name__ == "__main__":
    main()
