"""Times the watch-order counts (rsys_watch_order_*) on synthetic histories and prints one JSON line.

Assumed histories (recorded in the line): --users users, lengths log-normal with median --median and sigma --sigma, capped at --cap;
items drawn with Zipf(--zipf) popularity over a random permutation of the ids, deduplicated per user (first occurrence kept, as
project_earliest keeps it).  For each V: device seconds of the adds (upload + count, synchronous calls, the host's argument checks
included), pairs counted, pairs per second; the CSR export (count pass alone, then count + fill + copy-out) and a 10^6-pair gather.
The host path is the restatement's loops (tests/_media_relations_np.py get_watch_order) on --host-users users, scaled by pairs.
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats`.

  python tools/bench_watch_order.py [--users 2000000 --V 40000,120000 --median 60 --sigma 1.0 --cap 20000 --zipf 1.1]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def histories(rng, n_users, V, median, sigma, cap, zipf):
    """(offsets, items) of n_users synthetic projected histories"""
    L = np.minimum(np.round(np.exp(np.log(median) + sigma * rng.standard_normal(n_users))).astype(np.int64), cap)
    L = np.minimum(np.maximum(L, 0), V)
    n = int(L.sum())
    cdf = np.cumsum(1.0 / np.arange(1, V + 1) ** zipf)
    cdf /= cdf[-1]
    perm = rng.permutation(V).astype(np.int64)
    raw = perm[np.minimum(np.searchsorted(cdf, rng.random(n)), V - 1)]
    uid = np.repeat(np.arange(n_users, dtype=np.int64), L)
    _, first = np.unique(uid * V + raw, return_index=True)
    keep = np.sort(first)
    off = np.zeros(n_users + 1, np.int64)
    np.cumsum(np.bincount(uid[keep], minlength=n_users), out=off[1:])
    return off, raw[keep].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=2_000_000)
    ap.add_argument("--V", default="40000,120000")
    ap.add_argument("--median", type=float, default=60.0)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--cap", type=int, default=20000)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--batch", type=int, default=250_000, help="users per add call")
    ap.add_argument("--host-users", type=int, default=300)
    ap.add_argument("--csr-max-V", type=int, default=40000, help="largest V whose CSR is copied out in full (host memory)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _media_relations_np as ref
    from recommendersystem_amd import relations as rel
    import ctypes as C
    from recommendersystem_amd._lib import check, lib

    res = {"assumed": {"users": a.users, "lengths": f"lognormal(median {a.median}, sigma {a.sigma}) capped at {a.cap}",
                       "items": f"Zipf({a.zipf}) popularity, distinct per user", "users_per_add": a.batch}, "runs": []}
    for V in (int(x) for x in a.V.split(",")):
        rng = np.random.default_rng(V)
        batches = []
        for u0 in range(0, a.users, a.batch):
            batches.append(histories(rng, min(a.batch, a.users - u0), V, a.median, a.sigma, a.cap, a.zipf))
        lens = np.concatenate([np.diff(b[0]) for b in batches])
        pairs = int((lens * (lens - 1) // 2).sum())
        w = rel.WatchOrder(V)
        t0 = time.perf_counter()
        for off, items in batches:
            w.add((off, items))
        t_add = time.perf_counter() - t0
        run = {"V": V, "users": int(w.users()), "items": int(lens.sum()), "mean_len": float(lens.mean()), "max_len": int(lens.max()),
               "pairs": pairs, "add_s": t_add, "pairs_per_s": pairs / t_add, "band_bytes": V * ((V + 3) // 4 * 4) * 4}
        nnz = C.c_int64()
        t0 = time.perf_counter()
        check(lib().rsys_watch_order_csr(w.h, None, None, None, 0, C.byref(nnz)))
        run["csr_count_s"] = time.perf_counter() - t0
        run["nnz"] = nnz.value
        if V <= a.csr_max_V:
            t0 = time.perf_counter()
            ip, ix, vv = w.csr()
            run["csr_full_s"] = time.perf_counter() - t0
            assert int(vv.sum(dtype=np.int64)) == pairs
            del ip, ix, vv
        ga, gb = rng.integers(0, V, 10 ** 6), rng.integers(0, V, 10 ** 6)
        w.gather(ga, gb)
        t0 = time.perf_counter()
        w.gather(ga, gb)
        run["gather_1e6_s"] = time.perf_counter() - t0
        # the host path: the restatement's loops on a few users, scaled by pairs
        off, items = batches[0]
        nh = min(a.host_users, off.size - 1)
        ids, compact = np.unique(items[:off[nh]], return_inverse=True)      # (ids renumbered: the dense host matrix stays small)
        hist = [compact[off[u]:off[u + 1]].tolist() for u in range(nh)]
        hp = sum(len(h) * (len(h) - 1) // 2 for h in hist)
        t0 = time.perf_counter()
        ref.get_watch_order(hist, max(1, ids.size))
        th = time.perf_counter() - t0
        if hp:
            run["host_loops_pairs_per_s"] = hp / th
            run["host_loops_scaled_s"] = pairs / (hp / th)
        w.close()
        res["runs"].append(run)
        del batches
    print(json.dumps(res))


if __name__ == "__main__":
    main()
