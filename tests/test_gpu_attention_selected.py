"""GPU: the selected-query attention of the serving compact top (attn_sel_kernel, csrc/attention_serve.hip) through
rsys_op_attention_selected against the float64 reference of tests/_attention_np.py.  The kernel attends query token sel[i] to the keys of
its own row under the model's mask and writes compact row i; the reference computes every row of O and the test reads rows sel.

Inputs are make_users' rows (partial, empty and -- from T = 264 on -- full tile pairs) with ONE edit: token 5 of row 1 gets a user id of its
own, so that a query that sees only itself occurs.  Every test CHECKS that its selection holds what it is for (_selection): the first and
the last token of a row, a token in the partial last tile, two tokens of one tile, the same token twice, the lone token, a masked token
(tm != 0) with allowed and refused keys of its own user, both parities; n_sel = 1 and n_sel = 256.

Bounds: those of tests/test_gpu_attention_parity.py.  row_err per (selected token, head): fp32 e <= 1e-4 and whole-tensor <= 2e-5; bf16
e <= 2 E with E = the worst-row error of attn_emul_bf16 on the same rows, and whole-tensor <= 3e-2.  Each case prints a RATIO line.

Observed on an MI355X, lowest - highest over the nine shapes (also in DESIGN 4ze).  fp32: worst row e 3.6e-7 - 4.8e-7 (bound 1e-4), whole
tensor 8.4e-8 - 1.6e-7 (bound 2e-5).  bf16: e / E 0.68 - 0.82 (bound 2) with E 4.5e-3 - 5.7e-3, whole tensor 1.2e-3 - 2.4e-3 (bound 3e-2);
the ratio is below 1 because the kernel keeps its probabilities in fp32 where the emulated tile kernel packs them to bf16.  n_sel = 1 on
the lone token: e = 0 in both modes (its output is its own v).
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_np as an  # noqa: E402

pytestmark = pytest.mark.gpu

B = 2
LONE = (1, 5)   # (row, token) of the user with one token
# (T, H, KV, hd): every head_dim, H / KV = 1, 2, 4, 8, KV = 1, 2, 3, and the three row lengths; the last: 33 tiles, 64-bit map words
CASES = [(72, 1, 1, 16), (72, 8, 1, 64), (136, 4, 2, 32), (136, 12, 3, 16), (264, 2, 2, 128), (264, 8, 2, 64), (264, 8, 1, 128),
         (264, 6, 3, 32), (2112, 2, 1, 64)]


@functools.lru_cache(maxsize=None)
def _inputs(T, H, KV, hd, dtype):
    rng = np.random.default_rng(T * 101 + H * 7 + KV * 3 + hd + dtype)
    qkv = rng.standard_normal((B * T, (H + 2 * KV) * hd)).astype(np.float32)
    if dtype == 1:
        qkv = an.bf16_round(qkv)
    uid, tm = an.make_users(B, T, B + T + hd)
    uid = uid.copy(); tm = tm.copy()
    uid[LONE] = 400000; tm[LONE] = 0
    return qkv, uid, tm


@functools.lru_cache(maxsize=None)
def _reference(T, H, KV, hd, dtype):
    """(reference O, bf16 emulation's O or None), every token row: computed once per case, shared, never modified"""
    qkv, uid, tm = _inputs(T, H, KV, hd, dtype)
    q, k, v = qkv[:, :H * hd], qkv[:, H * hd:(H + KV) * hd], qkv[:, (H + KV) * hd:]
    dO = np.zeros((B * T, H * hd), np.float32)
    ref = an.attn_ref(q, k, v, uid, tm, dO, H, KV, hd)[0]
    emu = an.attn_emul_bf16(q, k, v, uid, tm, dO, H, KV, hd)[0] if dtype == 1 else None
    return ref, emu


def _masked_with_both(uid, tm):
    """flat index of a token with tm != 0 that has an allowed key other than itself and a refused key, both of its own user"""
    T = uid.shape[1]
    for b in range(uid.shape[0]):
        for t in np.nonzero(tm[b])[0]:
            own = uid[b] == uid[b, t]
            allowed = own & ((tm[b] == 0) | (tm[b] == tm[b, t]))
            if allowed.sum() >= 2 and (own & ~allowed).any():
                return b * T + int(t)
    return None


def _selection(uid, tm, n):
    """n flat token indices that hold every kind of the module docstring (n >= 16), checked; the rest random (duplicates allowed)"""
    T = uid.shape[1]
    mk = _masked_with_both(uid, tm)
    assert mk is not None, "no masked token with allowed and refused keys of its own user"
    lone = LONE[0] * T + LONE[1]
    assert (uid[LONE[0]] == uid[LONE]).sum() == 1
    head = [0, T - 1, T, 2 * T - 1, 1, 2, 70 % T, 70 % T, lone, mk]
    rng = np.random.default_rng(T + n)
    sel = np.array(head + rng.integers(0, B * T, n - len(head)).tolist(), np.int32)
    sel = sel[rng.permutation(n)]               # any order
    s = set(sel.tolist())
    assert {0, T - 1, T, 2 * T - 1} <= s                                        # first and last token of both rows
    if T % 64:
        assert any(v % T >= (T // 64) * 64 for v in s)                           # a token in the partial last tile
    assert 1 in s and 2 in s                                                     # two tokens of one tile
    assert (sel == 70 % T).sum() >= 2                                            # the same token twice
    assert lone in s and mk in s
    assert any(v % 2 == 0 for v in s) and any(v % 2 == 1 for v in s)             # item and action parity
    return sel


def _run(dtype, T, H, KV, hd, qkv, uid, tm, sel, extra=8):
    """one rsys_op_attention_selected call; O has `extra` rows behind n_sel that hold a NaN sentinel.  Returns the stored bits [n + extra][H hd]"""
    from recommendersystem_amd import _lib
    lib = _lib.lib()
    bf = dtype == 1
    et = np.uint16 if bf else np.float32
    ptrs = []

    def dev(a):
        p = C.c_void_p()
        assert lib.rsys_dev_alloc(C.byref(p), max(a.nbytes, 4)) == 0
        assert lib.rsys_dev_h2d(p, a.ctypes.data, a.nbytes) == 0
        ptrs.append(p)
        return p

    x = np.ascontiguousarray(qkv, np.float32)
    if bf:
        u = x.view(np.uint32)
        assert not (u & 0xFFFF).any()
        x = (u >> 16).astype(np.uint16)
    n = len(sel)
    o0 = np.zeros((n + extra, H * hd), et)
    o0[:] = 0x7FC0 if bf else np.nan
    d_qkv, d_uid, d_tm = dev(x), dev(np.ascontiguousarray(uid, np.int32)), dev(np.ascontiguousarray(tm, np.int32))
    d_sel, d_O = dev(np.ascontiguousarray(sel, np.int32)), dev(o0)
    rc = lib.rsys_op_attention_selected(dtype, B, T, H, KV, hd, d_qkv, d_uid, d_tm, n, d_sel, d_O)
    assert rc == 0, _lib.last_error()
    out = np.empty_like(o0)
    assert lib.rsys_dev_d2h(out.ctypes.data, d_O, out.nbytes) == 0
    for p in ptrs:
        lib.rsys_dev_free(p)
    return out


def _values(raw, bf):
    return (raw.astype(np.uint32) << 16).view(np.float32) if bf else raw


def _check(tag, raw, sel, ref, emu, H, bf):
    n = len(sel)
    a, b = _values(raw[:n], bf), ref[sel]
    e, (row, head) = an.row_err(a, b, H)
    g = float(np.abs(np.nan_to_num(a.astype(np.float64), nan=np.inf) - b).max() / np.abs(b).max())
    E = an.row_err(emu[sel], b, H)[0] if bf else 0.0
    bound, gbound = (2 * E, 3e-2) if bf else (1e-4, 2e-5)
    print(f"RATIO {tag} {'bf16' if bf else 'fp32'} O: e {e:.3e} at (compact row {row}, token {int(sel[row])}, head {head})  E {E:.3e}  "
          f"e/E {e / E if E else float('nan'):.2f}  whole-tensor {g:.3e}")
    assert e <= bound and g <= gbound, (tag, "row", e, "bound", bound, "whole-tensor", g, "bound", gbound)
    sent = raw[n:]
    fresh = np.empty_like(sent)
    fresh[:] = 0x7FC0 if bf else np.nan                      # what _run put there
    assert sent.size and sent.tobytes() == fresh.tobytes(), "the rows behind n_sel were written"


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("T,H,KV,hd", CASES)
def test_selected_rows_against_the_reference(T, H, KV, hd, dtype):
    """n_sel = 256 with every kind of selection, and n_sel = 1 on the lone token (it sees only itself: its output is its own v)"""
    qkv, uid, tm = _inputs(T, H, KV, hd, dtype)
    ref, emu = _reference(T, H, KV, hd, dtype)
    bf = dtype == 1
    sel = _selection(uid, tm, 256)
    raw = _run(dtype, T, H, KV, hd, qkv, uid, tm, sel)
    _check(f"sel256 T{T} H{H} KV{KV} hd{hd}", raw, sel, ref, emu, H, bf)
    lone = np.array([LONE[0] * T + LONE[1]], np.int32)
    raw1 = _run(dtype, T, H, KV, hd, qkv, uid, tm, lone)
    _check(f"sel1 T{T} H{H} KV{KV} hd{hd}", raw1, lone, ref, emu, H, bf)
    v = qkv[lone[0], (H + KV) * hd:].reshape(KV, 1, hd)
    np.testing.assert_array_equal(_values(raw1[:1], bf).reshape(KV, H // KV, hd), np.broadcast_to(v, (KV, H // KV, hd)))
    # compact row i depends on sel[i] alone: the row of the n_sel = 1 call is the lone token's row of the n_sel = 256 call, bit for bit
    i = int(np.nonzero(sel == lone[0])[0][0])
    assert raw1[0].tobytes() == raw[i].tobytes()


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("T,H,KV,hd", [(72, 8, 1, 64), (264, 6, 3, 32), (2112, 2, 1, 64)])
def test_permuting_the_selection_permutes_the_rows(T, H, KV, hd, dtype):
    qkv, uid, tm = _inputs(T, H, KV, hd, dtype)
    sel = _selection(uid, tm, 256)
    perm = np.random.default_rng(7).permutation(len(sel))
    a = _run(dtype, T, H, KV, hd, qkv, uid, tm, sel)
    b = _run(dtype, T, H, KV, hd, qkv, uid, tm, sel[perm])
    assert a[:len(sel)][perm].tobytes() == b[:len(sel)].tobytes()
    same = np.nonzero(sel == 70 % T)[0]                      # the same token twice: the same bits twice
    assert len(same) >= 2 and a[same[0]].tobytes() == a[same[1]].tobytes()
