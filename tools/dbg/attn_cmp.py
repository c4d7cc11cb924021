"""The attention outputs of two builds of the library on the same operands, bit for bit:

    python tools/dbg/attn_cmp.py <lib_a.so> <lib_b.so> [B T H KV hd dtype]

One child process per library (the switches and the library are per process) runs every case and stores its outputs; the parent
prints, per case and output, the number of elements whose bits differ, and exits 1 when there is one.  With a shape the one case is
  plain     rsys_op_attention: O, dqkv, lse (this child is also what tests/test_gpu_ops.py runs once per RSYS_ATTN_DMA setting)
and without one the cases are the shapes of the op-level parity tests (tests/test_gpu_attention_parity.py, and the shortest row of
64-bit map words of test_gpu_attention_long_rows.py), both dtypes, with and without q_active:
  train     rsys_op_attention_ex with shuffled RoPE positions (and, with q_active, one live query tile less per row): O, lse, dq|dk|dv
  selected  rsys_op_attention_selected on the same operands: the compact rows of 37 selected tokens (duplicates among them)
  cached    rsys_op_attention_cached and rsys_op_attention_cached_tiles at the shapes of tests/test_gpu_rank_cache_tiles_ops.py."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
TRAIN = [(2, 328, 2, 1, 64), (8, 328, 8, 4, 64), (2, 328, 4, 2, 32), (2, 328, 2, 2, 16), (1, 200, 2, 1, 128), (1, 2112, 2, 1, 16), (1, 2112, 2, 1, 64)]
# tests/test_gpu_rank_cache_tiles_ops.py: (row, first_tile, n_cand, slot, n_hist) of two rows of four tiles, and its (hd, H / KV, KV) cases
C_ROWS, C_T, C_SLOTS = 2, 256, 8
SEGMENTS = [[(0, 0, 1, 0, 0), (0, 2, 64, 1, 31), (1, 0, 31, 2, 1), (1, 1, 32, 3, 63), (1, 3, 32, 3, 63)],
            [(0, 0, 33, 4, 32), (1, 0, 1, 5, 33), (1, 1, 31, 4, 32), (1, 2, 1, 5, 33)]]
CACHED = [(hd, rep, 1) for hd in (16, 32, 64, 128) for rep in (1, 2)] + [(64, 2, 2), (32, 1, 3)]


def cases(argv):
    if argv:
        return [("plain",) + tuple(int(x) for x in argv[:6])]
    out = [("train",) + s + (dt, qa) for s in TRAIN for dt in (0, 1) for qa in (0, 1)]
    return out + [("cached", hd, rep, kv, dt) for hd, rep, kv in CACHED for dt in (0, 1)]


def parent(lib_a, lib_b, argv):
    outs = []
    for lib in (lib_a, lib_b):
        with tempfile.TemporaryDirectory() as d:
            f = os.path.join(d, "out.npz")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", lib, f] + argv)
            with np.load(f) as z:
                outs.append({k: z[k] for k in z.files})
    assert outs[0].keys() == outs[1].keys()
    bad = 0
    for k in outs[0]:
        a, b = outs[0][k], outs[1][k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        ua, ub = a.view(np.uint16 if a.itemsize == 2 else np.uint32), b.view(np.uint16 if b.itemsize == 2 else np.uint32)
        n = int((ua != ub).sum())
        bad += n
        rows = sorted(set(np.argwhere(ua != ub)[:, 0].tolist()))[:20] if n else ""
        print(f"{k}: {a.size} elements, {n} differ in their bits", f"(non-zero: {int((ua != 0).sum())})", rows)
    print("BIT-IDENTICAL" if bad == 0 else f"DIFFERENT: {bad} elements", f"over {len(outs[0])} outputs")
    return 0 if bad == 0 else 1


def child(lib_path, out, argv):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _attention_np import make_users
    from recommendersystem_amd import _lib
    _lib.LIB_PATH = lib_path
    lib = _lib.lib()
    ptrs = []

    def dev(a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert lib.rsys_dev_alloc(C.byref(p), max(a.nbytes, 16)) == 0
        assert lib.rsys_dev_h2d(p, a.ctypes.data, a.nbytes) == 0
        ptrs.append(p)
        return p

    def back(p, shape, t):
        o = np.empty(shape, t)
        assert lib.rsys_dev_d2h(o.ctypes.data, p, o.nbytes) == 0
        return o

    def pack(a, bf):   # float32, or its bf16 rounding (to nearest even, as the device does) as stored bits
        u = np.ascontiguousarray(a, np.float32).view(np.uint32)
        return ((u + (((u >> 16) & 1) + 0x7FFF)) >> 16).astype(np.uint16) if bf else u.view(np.float32)

    res = {}
    for case in cases(argv):
        if case[0] == "plain":   # outputs O, dqkv, lse as float32 VALUES: tests/test_gpu_ops.py drives this child with a shape
            _, B, T, H, KV, hd, dtype = case
            bf, et = dtype == 1, (np.uint16 if dtype == 1 else np.float32)
            rng = np.random.default_rng(1)
            Nq = (H + 2 * KV) * hd
            uid = np.sort(rng.integers(1, 4, (B, T)), axis=1).astype(np.int32).reshape(-1)
            tm = (rng.integers(1, 3, B * T) * (rng.random(B * T) < 0.2)).astype(np.int32)
            val = (lambda u: (u.astype(np.uint32) << 16).view(np.float32)) if bf else (lambda u: u)
            d_qkv, d_dO = dev(pack(rng.standard_normal((B * T, Nq)), bf)), dev(pack(rng.standard_normal((B * T, H * hd)), bf))
            d_O, d_g, d_lse = dev(np.zeros((B * T, H * hd), et)), dev(np.zeros((B * T, Nq), et)), dev(np.zeros((B, H, T), np.float32))
            f = 1.0 / (500000.0 ** (np.arange(0, hd, 2, dtype=np.float32) / hd))
            ang = np.outer(np.arange(T, dtype=np.float32), f)
            _lib.check(lib.rsys_op_attention(dtype, B, T, H, KV, hd, d_qkv, dev(uid), dev(tm), d_O, d_lse, d_dO, d_g, dev(np.cos(ang).astype(np.float32)),
                                             dev(np.sin(ang).astype(np.float32))))
            res.update(O=val(back(d_O, (B * T, H * hd), et)), dqkv=val(back(d_g, (B * T, Nq), et)), lse=back(d_lse, (B * H, T), np.float32))
        elif case[0] == "train":
            _, B, T, H, KV, hd, dtype, qa = case
            bf, et = dtype == 1, (np.uint16 if dtype == 1 else np.float32)
            name = f"train B{B} T{T} H{H} KV{KV} hd{hd} {'bf16' if bf else 'fp32'}{' q_active' if qa else ''}"
            rng = np.random.default_rng(B + T + hd)
            Nq, nt = (H + 2 * KV) * hd, (T + 63) // 64
            uid, tm = make_users(B, T, B + T + hd, "high" if T > 2048 else "low")
            qkv, dO = rng.standard_normal((B * T, Nq)), rng.standard_normal((B, T, H * hd))
            q_active = np.maximum(nt - 1 - (np.arange(B) % 2), 1).astype(np.int32)
            if qa:
                for b in range(B):
                    dO[b, 64 * q_active[b]:] = 0.0   # (the hook's contract: dO of the query tiles nobody reads is zero)
            rows = T + 16
            f = 1.0 / (500000.0 ** (np.arange(0, hd, 2, dtype=np.float32) / hd))
            ang = np.outer(np.arange(rows, dtype=np.float32), f)
            pos = rng.integers(0, rows, B * T).astype(np.int32)
            d_qkv, d_uid, d_tm = dev(pack(qkv, bf)), dev(uid), dev(tm)
            d_O, d_lse, d_g = dev(np.zeros((B * T, H * hd), et)), dev(np.zeros((B, H, T), np.float32)), dev(np.zeros((B * T, Nq), et))
            _lib.check(lib.rsys_op_attention_ex(dtype, B, T, H, KV, hd, d_qkv, d_uid, d_tm, d_O, d_lse, dev(pack(dO, bf)), d_g, dev(np.cos(ang).astype(np.float32)),
                                                dev(np.sin(ang).astype(np.float32)), dev(pos), rows, dev(q_active) if qa else None, None, None))
            res[name + " O"], res[name + " lse"] = back(d_O, (B * T, H * hd), et), back(d_lse, (B * H, T), np.float32)
            res[name + " dq|dk|dv"] = back(d_g, (B * T, Nq), et)
            if not qa:
                sel = rng.integers(0, B * T, 37).astype(np.int32)
                sel[5] = sel[4]
                d_c = dev(np.zeros((37, H * hd), et))
                _lib.check(lib.rsys_op_attention_selected(dtype, B, T, H, KV, hd, d_qkv, d_uid, d_tm, 37, dev(sel), d_c))
                res[name.replace("train", "selected") + " rows"] = back(d_c, (37, H * hd), et)
        else:
            _, hd, rep, KV, dtype = case
            bf, et, H = dtype == 1, (np.uint16 if dtype == 1 else np.float32), KV * rep
            name = f"cached hd{hd} H{H} KV{KV} {'bf16' if bf else 'fp32'}"
            rng = np.random.default_rng(7000 + 100 * hd + 10 * rep + 2 * KV + dtype)
            Nq, kvw, No = (H + 2 * KV) * hd, 2 * KV * hd, H * hd
            d_qkv = dev(pack(rng.standard_normal((C_ROWS * C_T, Nq)), bf))
            d_cache = dev(pack(rng.standard_normal((C_SLOTS, C_T, kvw)), bf))
            for i, seg in enumerate(SEGMENTS):
                segs = np.array(seg, np.int32)
                d_O = dev(np.zeros((C_ROWS * C_T, No), et))
                _lib.check(lib.rsys_op_attention_cached_tiles(dtype, C_ROWS, C_T, H, KV, hd, d_qkv, d_cache, C_SLOTS, 0, len(seg), segs.ctypes.data, d_O))
                res[f"{name} tiles {'ab'[i]}"] = back(d_O, (C_ROWS * C_T, No), et)
                # the row form: row r of the same qkv with the slot and the counts of segment r
                d_O = dev(np.zeros((C_ROWS * C_T, No), et))
                _lib.check(lib.rsys_op_attention_cached(dtype, C_ROWS, C_T, H, KV, hd, d_qkv, d_cache, C_SLOTS, dev(segs[:C_ROWS, 3].copy()), dev(segs[:C_ROWS, 4].copy()),
                                                        dev(segs[:C_ROWS, 2].copy()), d_O))
                res[f"{name} rows {'ab'[i]}"] = back(d_O, (C_ROWS * C_T, No), et)
        for p in ptrs:
            lib.rsys_dev_free(p)
        ptrs.clear()
    np.savez(out, **res)


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], sys.argv[4:])
    elif len(sys.argv) >= 3:
        sys.exit(parent(sys.argv[1], sys.argv[2], sys.argv[3:]))
    else:
        sys.exit(__doc__)
