"""One rsys_op_attention_ex call on given operands: run_attention() for tests/test_gpu_attention_parity.py, and as a program the worker
of its kernel-variant test -- the RSYS_ATTN_* switches are read once per process, so every variant is a process of its own:
python _attention_worker.py <in.npz> <out.npz> <repository root>."""
import ctypes as C
import sys

import numpy as np


def _pack(x, bf):
    x = np.ascontiguousarray(x, np.float32)
    if not bf:
        return x
    u = x.view(np.uint32)
    assert not (u & 0xFFFF).any(), "bf16 operands must be bf16-representable"
    return (u >> 16).astype(np.uint16)


def _unpack(raw, bf):
    return (raw.astype(np.uint32) << 16).view(np.float32) if bf else raw


def run_attention(dtype, H, KV, hd, qkv, uid, tm, dO, cos, sin, pos=None, q_active=None, amax=False, nan_out=False, pos_pad=64):
    """qkv [B*T][(H+2KV)*hd], dO [B*T][H*hd] float32 (bf16-representable when dtype == 1), uid / tm [B][T], cos / sin [rows][hd/2],
    pos [B][T] or None, q_active [B] or None.  nan_out: O and lse hold NaN before the call.  The position buffer is pos_pad entries
    longer than B*T (copies of its last entry).  Returns a dict: O, dq, dk, dv (float32 values), lse, raw_O / raw_dqkv (the stored bits)
    and with amax the four maxima over the shards (O, dq, dk, dv)."""
    from recommendersystem_amd import _lib
    lib = _lib.lib()
    bf = dtype == 1
    B, T = uid.shape
    Nq = (H + 2 * KV) * hd
    et = np.uint16 if bf else np.float32
    ptrs = []

    def dev(a):
        p = C.c_void_p()
        assert lib.rsys_dev_alloc(C.byref(p), max(a.nbytes, 4)) == 0
        assert lib.rsys_dev_h2d(p, a.ctypes.data, a.nbytes) == 0
        ptrs.append(p)
        return p

    def back(p, shape, t):
        out = np.empty(shape, t)
        assert lib.rsys_dev_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    d_qkv, d_dO = dev(_pack(qkv, bf)), dev(_pack(dO, bf))
    d_uid, d_tm = dev(np.ascontiguousarray(uid, np.int32)), dev(np.ascontiguousarray(tm, np.int32))
    d_cos, d_sin = dev(np.ascontiguousarray(cos, np.float32)), dev(np.ascontiguousarray(sin, np.float32))
    d_pos = None
    if pos is not None:
        flat = np.ascontiguousarray(pos, np.int32).reshape(-1)
        d_pos = dev(np.concatenate([flat, np.full(pos_pad, flat[-1], np.int32)]))
    d_qa = dev(np.ascontiguousarray(q_active, np.int32)) if q_active is not None else None
    o0 = np.zeros((B * T, H * hd), et)
    if nan_out:
        o0[:] = 0x7FC0 if bf else np.nan          # (0x7FC0: a bf16 quiet NaN)
    d_O = dev(o0)
    d_lse = dev(np.full((B, H, T), np.nan if nan_out else 0.0, np.float32))
    d_g = dev(np.zeros((B * T, Nq), et))
    d_af = dev(np.zeros(64 * 32, np.float32)) if amax else None
    d_ab = dev(np.zeros(64 * 32, np.float32)) if amax else None
    rc = lib.rsys_op_attention_ex(dtype, B, T, H, KV, hd, d_qkv, d_uid, d_tm, d_O, d_lse, d_dO, d_g, d_cos, d_sin, d_pos, cos.shape[0],
                                  d_qa, d_af, d_ab)
    assert rc == 0, _lib.last_error()
    res = {"raw_O": back(d_O, (B * T, H * hd), et), "raw_dqkv": back(d_g, (B * T, Nq), et), "lse": back(d_lse, (B, H, T), np.float32)}
    if amax:
        af, ab = back(d_af, (64, 32), np.float32), back(d_ab, (64, 32), np.float32)
        res["amax"] = np.array([af[:, 0].max(), ab[:, 0].max(), ab[:, 1].max(), ab[:, 2].max()], np.float32)
    for p in ptrs:
        lib.rsys_dev_free(p)
    G = _unpack(res["raw_dqkv"], bf)
    res.update(O=_unpack(res["raw_O"], bf), dq=G[:, :H * hd], dk=G[:, H * hd:(H + KV) * hd], dv=G[:, (H + KV) * hd:])
    return res


if __name__ == "__main__":
    src, out, root = sys.argv[1:4]
    sys.path.insert(0, root)
    a = np.load(src)
    r = run_attention(int(a["dtype"]), int(a["H"]), int(a["KV"]), int(a["hd"]), a["qkv"], a["uid"], a["tm"], a["dO"], a["cos"], a["sin"], a["pos"])
    np.savez(out, **r)
