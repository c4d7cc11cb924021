"""CPU: the host side of rsys_batch_upload / rsys_batch_upload_trimmed -- the check of a batch and its packing into the staging
buffer (csrc/model_batch.hip: batch_check, batch_pack) -- through rsys_debug_batch_pack, which runs exactly those two on a caller's
buffer without a model or a device.  max_rows 3 and max_sequence_length 12 give N = 36 interactions: neither 4 N nor N is a multiple of
64, so the 64-byte steps of the layout carry padding."""
import ctypes as C
import os

import numpy as np
import pytest

ROWS_MAX, S, TA, V0, V1, VS, VG, VSRC = 3, 12, 24, 30, 50, 9, 4, 4
V = V0 + V1
LIMITS = np.array([ROWS_MAX, S, TA, V, V0, V1, VS, VG, VSRC], np.int32)
OK, ARG = 0, -1
FILL = 0xAB
CAP = 8192
# the arrays in the order the layout places them: (name, numpy dtype, elements per interaction)
ORDER = ([("time", np.float64, 1)] + [(n, np.int32, 1) for n in ("userid", "token_mask_ids", "gender", "source", "matchedid", "status")]
         + [("rating", np.float32, 1), ("progress", np.float32, 1)]
         + [(f"{w}{k}", np.int32 if w == "position" else np.float32, 1) for k in range(6) for w in ("label", "weight", "position")]
         + [("watch_mask", np.uint8, 1), ("rating_mask", np.uint8, 1), ("rope", np.int32, 2)])
INPUTS = [n for n, _, _ in ORDER[:9]]
TARGETS = [n for n, _, _ in ORDER[9:27]]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    from recommendersystem_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


def make_arrays(rows, seed, masks=True, rope=True, status_targets=False, live=S):
    """a valid batch of `rows` rows; columns >= live of every row are padding (zeros, userid 0)"""
    rng = np.random.default_rng(seed)
    n = rows * S
    a = {"time": rng.uniform(1e9, 2e9, n), "userid": rng.integers(1, 1 << 19, n), "token_mask_ids": rng.integers(0, 4096, n),
         "gender": rng.integers(-1, VG + 1, n), "source": rng.integers(-1, VSRC + 1, n), "matchedid": rng.integers(-1, V, n),
         "status": rng.integers(-1, VS + 1, n), "rating": rng.uniform(0, 10, n), "progress": rng.uniform(0, 1, n)}
    for k in range(6):
        if k % 3 == 2 and not status_targets:
            continue
        a[f"label{k}"] = rng.uniform(0, 1, n); a[f"weight{k}"] = rng.uniform(0, 1, n)
        a[f"position{k}"] = rng.integers(0, V0 if k < 3 else V1, n)
    if masks:
        a["watch_mask"] = rng.integers(0, 2, n); a["rating_mask"] = rng.integers(0, 2, n)
    if rope:
        a["rope_input_pos"] = rng.integers(0, TA // 2, n)
    dt = {n_: d for n_, d, _ in ORDER}
    dt["rope_input_pos"] = np.int32
    a = {k: np.ascontiguousarray(v, dt[k]) for k, v in a.items()}
    for v in a.values():
        v.reshape(rows, S)[:, live:] = 0
    return a


def c_batch(a, rows):
    from recommendersystem_amd import _lib
    b = _lib.rsys_batch()
    b.rows = rows
    for name in INPUTS + ["watch_mask", "rating_mask", "rope_input_pos"]:
        if name in a:
            setattr(b, name, a[name].ctypes.data)
    for k in range(6):
        for w in ("label", "weight", "position"):
            if f"{w}{k}" in a:
                getattr(b, w)[k] = a[f"{w}{k}"].ctypes.data
    return b


def pack(L, a, rows, row_len, batch=True):
    from recommendersystem_amd import _lib
    buf = np.full(CAP, FILL, np.uint8)
    off = np.full(30, -1, np.int64)
    total, distinct = C.c_int64(-1), C.c_int32(-1)
    b = c_batch(a, rows)
    rc = L.rsys_debug_batch_pack(C.byref(b) if batch else None, LIMITS.ctypes.data, row_len, buf.ctypes.data, buf.size, off.ctypes.data,
                                 C.byref(total), C.byref(distinct))
    return rc, buf, off, total.value, distinct.value, (_lib.last_error() if rc else "")


def expected(a, rows, row_len):
    """name -> the bytes its place must hold (absent arrays: none)"""
    out = {}
    cut = lambda x: np.ascontiguousarray(x.reshape(rows, S)[:, :row_len])
    for name in INPUTS + (TARGETS + ["watch_mask", "rating_mask"] if row_len == S else []):
        if name in a:
            out[name] = cut(a[name]).view(np.uint8).reshape(-1)
    if "rope_input_pos" in a:
        p = cut(a["rope_input_pos"]).reshape(-1)
        out["rope"] = np.stack([2 * p, 2 * p + 1], 1).astype(np.int32).view(np.uint8).reshape(-1)
    return out


def check_packed(a, rows, row_len, buf, off, total, distinct):
    n = rows * row_len
    size = [n * np.dtype(d).itemsize * per for _, d, per in ORDER]
    assert off[0] == 0
    for i in range(30):
        assert off[i] % 64 == 0
        end = off[i] + size[i]
        assert end <= (off[i + 1] if i + 1 < 30 else total)          # ascending, no overlap
        assert (off[i + 1] if i + 1 < 30 else total) - end < 64      # back to back at 64-byte steps
    assert total == off[29] + -(-size[29] // 64) * 64 and total <= CAP
    want = expected(a, rows, row_len)
    written = np.zeros(CAP, bool)
    for i, (name, _, _) in enumerate(ORDER):
        if name in want:
            assert np.array_equal(buf[off[i]:off[i] + size[i]], want[name]), name
            written[off[i]:off[i] + size[i]] = True
    assert (buf[~written] == FILL).all(), "padding and the places of absent arrays stay unwritten"
    ids = a["matchedid"].reshape(rows, S)[:, :row_len]
    assert distinct == len(np.unique(ids[ids >= 0])) + 1


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("rows", [1, 3])
def test_ordinary_form(L, rows, masks, rope):
    a = make_arrays(rows, 10 * rows + 2 * masks + rope, masks=masks, rope=rope)          # (the two status-target triples absent)
    rc, buf, off, total, distinct, err = pack(L, a, rows, S)
    assert rc == OK, err
    check_packed(a, rows, S, buf, off, total, distinct)


def test_ordinary_form_with_status_targets(L):
    a = make_arrays(3, 5, status_targets=True)
    rc, buf, off, total, distinct, err = pack(L, a, 3, S)
    assert rc == OK, err
    check_packed(a, 3, S, buf, off, total, distinct)


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("row_len", [8, 4])
def test_trimmed_form(L, row_len, rope):
    a = make_arrays(3, 20 + row_len + rope, masks=True, rope=rope, live=row_len - 1)
    rc, buf, off, total, distinct, err = pack(L, a, 3, row_len)
    assert rc == OK, err
    check_packed(a, 3, row_len, buf, off, total, distinct)          # (targets and masks are given and still not written)


# ---------------------------------------------------------------- rejections: one bad value each
def rejected(L, a, rows, row_len, message, batch=True):
    rc, buf, off, total, distinct, err = pack(L, a, rows, row_len, batch)
    assert rc == ARG, (rc, err)
    assert err.endswith(" : " + message), err
    assert (buf == FILL).all(), "a rejected batch writes nothing"


RANGES = [("matchedid", -2, V, "matchedid out of range"), ("userid", -1, 1 << 19, "userid must be in [0, 2^19)"),
          ("token_mask_ids", -1, 4096, "token_mask_ids must be in [0, 4096)"), ("status", -2, VS + 1, "status out of range"),
          ("gender", -2, VG + 1, "gender out of range"), ("source", -2, VSRC + 1, "source out of range"),
          ("rope_input_pos", -1, TA // 2, "rope_input_pos out of range")]
ROW_LEN_MSG = "trimmed upload: row_len % 4 == 0 and 4 <= row_len <= max_sequence_length"


@pytest.mark.parametrize("field,below,above,message", RANGES)
@pytest.mark.parametrize("row_len", [S, 8])
def test_out_of_range_values_are_rejected(L, row_len, field, below, above, message):
    for bad, at in ((below, 0), (above, 2 * S + row_len - 3)):          # first interaction; last row, inside the packed columns
        a = make_arrays(3, 40, live=row_len - 2)
        a[field][at] = bad
        rejected(L, a, 3, row_len, message)
    a = make_arrays(3, 40, live=row_len - 2)
    a[field][at] = above - 1                                            # the largest value allowed
    assert pack(L, a, 3, row_len)[0] == OK


def test_ordinary_only_rejections(L):
    a = make_arrays(2, 50)
    a["label2"] = a["label0"]                                           # a half-given status triple counts as given
    rejected(L, a, 2, S, "target arrays must not be null")
    for name in ("label0", "weight1", "position3", "weight4"):
        a = make_arrays(2, 50)
        del a[name]
        rejected(L, a, 2, S, "target arrays must not be null")
    for k, lim, message in ((0, V0, "manga target position out of range"), (1, V0, "manga target position out of range"),
                            (3, V1, "anime target position out of range"), (4, V1, "anime target position out of range")):
        for bad in (-1, lim):
            a = make_arrays(2, 51)
            a[f"position{k}"][S + 5] = bad
            rejected(L, a, 2, S, message)
    a = make_arrays(2, 52)
    del a["rating_mask"]
    rejected(L, a, 2, S, "watch_mask and rating_mask come together")
    a = make_arrays(2, 52)
    del a["watch_mask"]                                                 # a rating mask alone is accepted, as it always was
    rc, buf, off, total, distinct, err = pack(L, a, 2, S)
    assert rc == OK, err
    check_packed(a, 2, S, buf, off, total, distinct)


def test_trimmed_only_rejections(L):
    a = make_arrays(3, 60, live=8)
    a["userid"][S + 8] = 7
    rejected(L, a, 3, 8, "trimmed upload: a live event (userid != 0) at or behind column row_len")
    a["userid"][S + 8] = 0
    a["userid"][3 * S - 1] = 7                                          # the last column of the last row
    rejected(L, a, 3, 8, "trimmed upload: a live event (userid != 0) at or behind column row_len")
    for field, below, above, _ in RANGES:
        if field == "userid":
            continue
        a = make_arrays(3, 61, live=8)
        a[field][S + 9] = above                                         # behind row_len: never read
        rc, buf, off, total, distinct, err = pack(L, a, 3, 8)
        assert rc == OK, (field, err)
        check_packed(a, 3, 8, buf, off, total, distinct)
    a = make_arrays(3, 62, live=3)
    del a["label0"], a["position4"], a["rating_mask"]                   # neither targets nor masks are looked at
    assert pack(L, a, 3, 4)[0] == OK
    for row_len in (0, 6, 16, -4):
        rejected(L, make_arrays(3, 63, live=0), 3, row_len, ROW_LEN_MSG)


@pytest.mark.parametrize("row_len", [S, 8])
def test_whole_call_rejections(L, row_len):
    a = make_arrays(3, 70, live=row_len)
    rejected(L, a, 3, row_len, "null batch", batch=False)
    rejected(L, a, 0, row_len, "batch rows must be in [1, max_rows]")
    big = {k: np.concatenate([v, v[:S]]) for k, v in a.items()}
    rejected(L, big, 4, row_len, "batch rows must be in [1, max_rows]")
    for name in INPUTS:
        a = make_arrays(3, 70, live=row_len)
        del a[name]
        rejected(L, a, 3, row_len, "batch arrays must not be null")


def test_a_buffer_below_the_layout_is_a_state_error(L):
    from recommendersystem_amd import _lib
    a = make_arrays(3, 80)
    b = c_batch(a, 3)
    buf = np.full(CAP, FILL, np.uint8)
    off = np.zeros(30, np.int64); total, distinct = C.c_int64(), C.c_int32()
    rc, _, _, need, _, _ = pack(L, a, 3, S)
    assert rc == OK
    rc = L.rsys_debug_batch_pack(C.byref(b), LIMITS.ctypes.data, S, buf.ctypes.data, need - 1, off.ctypes.data, C.byref(total), C.byref(distinct))
    assert rc == -3 and "staging buffer too small" in _lib.last_error()
    assert (buf == FILL).all()
