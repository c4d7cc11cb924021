"""CPU: the host side of inference on trimmed rows -- serve.trim_length, the token-index translation the library
applies on a trimmed batch (restated in tests/_trim_util.py; the library's own code is
reached by the GPU tests), and the premise of the exactness argument: every row serve.build_batch and serve.render_pack build is a
live prefix (userid != 0) followed by padding only (every array zero, userid 0)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _trim_util as tu  # noqa: E402

COLS = ("userid", "rope_input_pos", "token_mask_ids", "gender", "source", "matchedid", "status", "time", "rating", "progress")


def test_trim_length():
    from recommendersystem_amd import serve
    for live, want in tu.LIVE_TO_ROW_LEN.items():
        assert serve.trim_length(live, tu.S_TEST) == want
    assert serve.trim_length(0, 128) == 32 and serve.trim_length(1, 128) == 32          # (an empty row still runs one tile)
    assert serve.trim_length(1000 + 1, 2048) == 1024 and serve.trim_length(1030 + 1, 2048) == 1056
    assert serve.trim_length(5000, 2048) == 2048 and serve.trim_length(10, 16) == 16    # clamped to S
    for live in range(1, 300):
        rl = serve.trim_length(live, 256)
        assert rl % 32 == 0 and rl >= min(live, 256) and rl - 32 < live and rl <= 256


def test_token_index_translation():
    from recommendersystem_amd import serve
    S, rl = 128, 32
    idx = [0, 63, 2 * S + 7, 3 * 2 * S + 2 * rl - 1]
    assert tu.translate_token_index(idx, S, rl).tolist() == [0, 63, 2 * rl + 7, 3 * 2 * rl + 2 * rl - 1]
    assert tu.translate_token_index(idx, S, S).tolist() == idx
    with pytest.raises(ValueError):
        tu.translate_token_index([2 * rl], S, rl)            # the first dropped token of row 0
    with pytest.raises(ValueError):
        tu.translate_token_index([2 * S + 2 * rl], S, rl)


def _assert_dead_suffix(d, live_per_row):
    uid = np.asarray(d["userid"])
    for r, live in enumerate(live_per_row):
        assert (uid[r, :live] != 0).all(), (r, live)
        for k in COLS:
            assert not np.asarray(d[k])[r, live:].any(), (k, r)


@pytest.mark.parametrize("task", ["retrieval", "ranking"])
def test_build_batch_rows_are_a_live_prefix_and_padding(task):
    from recommendersystem_amd import serve
    cfg, V = tu.config()
    S = cfg["max_sequence_length"]
    rng = np.random.default_rng(3)
    hist = [0, 3, 31, 32, 90, S + 40]
    users = [tu.user_with_history(rng, nh, [int(x) for x in rng.integers(1, V[1], size=1 + i)]) for i, nh in enumerate(hist)]
    mul, mri = (S, 0) if task == "retrieval" else (S // 2, S - S // 2)
    d = serve.build_batch(users, task, 1, V[0], mul, mri)
    kept = [min(nh, mul - 1) for nh in hist]
    live = [k + (1 if task == "retrieval" else len(u["ranking_items"])) for k, u in zip(kept, users)]
    _assert_dead_suffix(d, live)
    assert serve.live_columns(d) == max(live)
    assert serve.live_columns({"userid": np.zeros((2, S), np.int32)}) == 0
    # the tokens `predict` selects lie inside every row length that covers the live columns
    index, _ = serve._selected_tokens(users, task, S, mul)
    rl = serve.trim_length(max(live), S)
    moved = tu.translate_token_index(index, S, rl)
    assert (moved % (2 * rl) == np.asarray(index) % (2 * S)).all()


@pytest.mark.parametrize("full", [False, True])
def test_render_pack_rows_are_a_live_prefix_and_padding(full):
    from recommendersystem_amd import serve
    cfg, V = tu.config()
    S = cfg["max_sequence_length"]
    rng = np.random.default_rng(5)
    hist = [0, 7, 70, S + 9]
    states = [dict(medium=i % 2, items=[], users=[dict(user=tu.user_with_history(rng, nh, []))]) for i, nh in enumerate(hist)]
    args = serve.render_pack(states, {"offset": 0, "limit": 10}, S, V[0], full_history=full)
    _assert_dead_suffix(args["retrieval_rows"], [min(nh, S - 1) + 1 for nh in hist])
    assert (args["retrieval_token"] // 2 + 1 == [min(nh, S - 1) + 1 for nh in hist]).all()
    if not full:
        _assert_dead_suffix(args["ranking_prefix"], [min(nh, S // 2 - 1) for nh in hist])
