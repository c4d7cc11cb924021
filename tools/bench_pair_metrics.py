"""Item-similarity catalogue ranks on the device (rsys_sim_pair_ranks) against the host path it replaces (the numpy
restatement of pairwise_metrics.jl: a masked fp32 Gram row and a full stable sort per source) and against the single-target count of
rsys_op_target_rank run once per target over the same score slab.

The reference's pair files are not available, so the shape is ASSUMED: V = 80 000 items, E = 1024, test-mask density 0.02 (bit rows built
from ANDs of random words: 1/64 + 1/256 = 0.0195), 20 000 distinct sources, targets per source log-normal with median 20 (sigma 1)
capped at 2000 and drawn from the source's unmasked items, a random unit-norm export.  Wall times, median of --reps after --warmup.  The
host path is timed on --host-sources sources in one thread and scaled to all sources and to 16 cores.  The per-kernel split comes from a
`rocprofv3 --kernel-trace --stats` run of this script.

    python tools/bench_pair_metrics.py --out profiles/pair_metrics_bench.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3


def mask_bits(V, rng, rows_per_block=4000):
    """bit rows [V][ceil(V / 32)] of density 1/64 + 1/256 - 1/16384"""
    W = (V + 31) // 32
    out = np.empty((V, W), np.uint32)
    for r0 in range(0, V, rows_per_block):
        n = min(rows_per_block, V - r0)
        def word():
            return rng.integers(0, 1 << 32, (n, W), dtype=np.uint32)
        a = word()
        for _ in range(5):
            a &= word()
        b = word()
        for _ in range(7):
            b &= word()
        out[r0:r0 + n] = a | b
    if V % 32:
        out[:, -1] &= np.uint32((1 << (V % 32)) - 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, default=80000)
    ap.add_argument("--E", type=int, default=1024)
    ap.add_argument("--sources", type=int, default=20000)
    ap.add_argument("--host-sources", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slab-targets", default="1,4,16,20,64,256,2000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import _pairwise_metrics_np as pm
    from recommendersystem_amd import similarity as sim
    from recommendersystem_amd._lib import check, lib
    V, E = a.V, a.E
    rng = np.random.default_rng(1)
    emb = rng.standard_normal((V, E), dtype=np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    bits = mask_bits(V, rng)
    cfg = sim.training_config({0: V}, embed_dim=E, batch_size=1, items_per_query=1)
    model = sim.LTRModel(cfg, 0, np.zeros((V, 64), np.float32), dtype="fp32", dropout=0.0)
    model.set_export(emb)
    check(lib().rsys_sim_testmask_set(model.h, bits.view(np.int32).ctypes.data))
    sources = rng.choice(V, a.sources, replace=False)
    counts = np.minimum(2000, np.maximum(1, np.round(np.exp(rng.normal(np.log(20.0), 1.0, a.sources))).astype(np.int64)))
    targets = []
    for s, n in zip(sources, counts):
        cand = np.flatnonzero(np.unpackbits(bits[s].view(np.uint8), bitorder="little")[:V])
        cand = cand[cand != s]
        targets.append(rng.choice(cand, min(int(n), len(cand)), replace=False))
    total = int(sum(len(t) for t in targets))
    res = dict(V=V, E=E, sources=a.sources, targets=total, mean_targets=round(total / a.sources, 2), median_targets=float(np.median(counts)),
               mask_density=round(float(np.unpackbits(bits[:64].view(np.uint8)).mean()), 5), assumed_shape=True)

    ranks = [None]

    def device():
        ranks[0] = model.pair_ranks(sources, targets)
    res["device_ms"] = round(timed(device, a.warmup, a.reps), 2)
    res["device_us_per_source"] = round(1e3 * res["device_ms"] / a.sources, 2)
    chunks = (a.sources + 255) // 256
    res["chunks"] = chunks
    res["gemm_gflop_per_chunk"] = round(2.0 * 256 * V * E / 1e9, 2)

    # the host path: the restatement's row and sort, one thread, a few sources; its ranks must be the device's wherever the fp32 sums agree
    hs = sources[:a.host_sources]
    mrows = np.unpackbits(bits[hs].view(np.uint8), axis=1, bitorder="little")[:, :V].astype(np.float32)

    def host():
        for j, s in enumerate(hs):
            row = (emb @ emb[s]) * mrows[j]
            pm.ranked_items(row, int(s))
    t_host = timed(host, 0, 1)
    res["host_ms_per_source_one_thread"] = round(t_host / len(hs), 2)
    res["host_path_ms_one_thread"] = round(t_host / len(hs) * a.sources, 0)
    res["host_path_ms_16_cores"] = round(t_host / len(hs) * a.sources / 16, 0)
    res["speedup_vs_host_16_cores"] = round(res["host_path_ms_16_cores"] / res["device_ms"], 1)
    agree = []
    for j, s in enumerate(hs):
        v = model.pair_scores([s])[0]
        agree.append(bool(np.array_equal(pm.ranks_of(v, int(s), targets[j]), ranks[0][j])))
    res["ranks_equal_host_order_on_device_rows"] = all(agree)

    # the counts alone on one slab [256][V] of masked score rows: the multi-target pass against the single-target pass once per target
    L = lib()
    rows = 256
    slab = model.pair_scores(sources[:rows])
    ld = (V + 7) // 8 * 8
    host_slab = np.full((rows, ld), np.nan, np.float32)
    host_slab[:, :V] = slab
    ptrs = []
    for nbytes in (host_slab.nbytes, rows * 4, rows * 4):
        p = C.c_void_p()
        check(L.rsys_dev_alloc(C.byref(p), nbytes))
        ptrs.append(p)
    check(L.rsys_dev_h2d(ptrs[0], host_slab.ctypes.data, host_slab.nbytes))
    self_ids = np.ascontiguousarray(sources[:rows], np.int32)
    one = np.ascontiguousarray([t[0] for t in targets[:rows]], np.int32)
    check(L.rsys_dev_h2d(ptrs[1], one.ctypes.data, one.nbytes))
    t_single = timed(lambda: check(L.rsys_op_target_rank(ptrs[0], ld, rows, V, ptrs[1], ptrs[2])), 2, 9)
    res["slab_bytes"] = int(rows * V * 4)
    res["single_target_call_ms"] = round(t_single, 4)
    multi = {}
    for T in (int(x) for x in a.slab_targets.split(",")):
        off = np.arange(rows + 1, dtype=np.int64) * T
        tid = np.ascontiguousarray(rng.integers(0, V, rows * T), np.int32)
        out = np.zeros(rows * T, np.int32)
        multi[T] = round(timed(lambda: check(L.rsys_op_pair_ranks(ptrs[0], ld, rows, V, self_ids.ctypes.data, off.ctypes.data,
                                                                  tid.ctypes.data, out.ctypes.data)), 2, 9), 4)
    res["multi_target_call_ms_by_targets_per_row"] = multi
    res["single_target_loop_ms_by_targets_per_row"] = {T: round(T * t_single, 3) for T in multi}
    for p in ptrs:
        L.rsys_dev_free(p)
    model.close()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
