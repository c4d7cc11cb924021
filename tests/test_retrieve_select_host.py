"""Host: the numpy side of the retrieval selection tests (tests/_retrieve_np.py) checked on its own, without a GPU: the float32
restatement of the log-sum-exp kernels' fold order against fp64 (its worst error is what the GPU tolerance is made of), the restated
rank bounds of the windowed select against their definition, and the named windows on the populations that must have all of them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _retrieve_np as rn  # noqa: E402


def test_lse_restatement_against_fp64():
    """Worst |restated - fp64| per kind of row over every shape the GPU test runs; the bound in _retrieve_np is this measurement rounded
    up, and must not be more than twice what is measured (a stale, loose figure would loosen the GPU tolerance)."""
    worst = {k: 0.0 for k in rn.LSE_KINDS}
    for V in rn.LSE_VS:
        for rows in rn.LSE_ROWS:
            z, kinds = rn.lse_case(V, rows)
            got, ref = rn.lse_restated(z), rn.lse_fp64(z)
            assert np.isfinite(ref).all() and np.isfinite(got).all(), (V, rows)
            err = np.abs(got.astype(np.float64) - ref)
            for r, k in enumerate(kinds):
                worst[k] = max(worst[k], float(err[r]))
    print("lse restatement worst |error| per kind:", {k: f"{v:.3e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= rn.LSE_RESTATED_ERR[k] <= 2 * v, (k, v, rn.LSE_RESTATED_ERR[k])


def test_lse_restatement_special_rows():
    z = np.full((2, 300), -np.inf, np.float32)
    z[1, 299] = 2.5                                             # every lane but one sees -inf only
    got = rn.lse_restated(z)
    assert np.isneginf(got[0]) and got[1] == np.float32(2.5)
    big = np.full((1, 70), 88.9, np.float32)                    # exp overflows without the max subtraction
    assert abs(float(rn.lse_restated(big)[0]) - (float(np.float32(88.9)) + np.log(70.0))) < 1e-5


@pytest.mark.parametrize("kind", ["digit_edges", "ulp", "special", "zeros"])
def test_select_bound_is_the_top_c_set(kind):
    rng = np.random.default_rng(3)
    x = rn._rows(kind, 3, 200, rng)
    for row in x:
        keys = rn.score_keys(row)
        order = rn.full_order(row)
        for c in range(0, order.size + 2):
            T, need = rn.select_bound(keys, c)
            above = np.flatnonzero(keys > T)
            ties = np.flatnonzero((keys == T) & (keys != 0))[:need]
            assert need >= 0 and sorted(np.concatenate([above, ties]).tolist()) == sorted(order[:c].tolist()), (kind, c, hex(T), need)


@pytest.mark.parametrize("V", [1025, 4097, 9500, 119999])
def test_digit_edges_rows_have_every_named_window(V):
    rng = np.random.default_rng(V)
    x = rn._rows("digit_edges", 5 if V < 100000 else 3, V, rng)
    for row in x:
        order = rn.full_order(row)
        W = rn.named_windows(row, order)
        assert set(W) == set(rn.WINDOW_NAMES), set(rn.WINDOW_NAMES) - set(W)
        for name, (start, length) in W.items():
            assert start >= 0 and 1 <= length <= rn.RT_WIN, name
        (te, ne), (ts, ns) = rn.expect_bounds(row, *W["inside_largest"]).tolist()
        assert te == ts and 0 < ns < ne                                             # one key, both exact
        (te, ne), (ts, ns) = rn.expect_bounds(row, *W["block_start"]).tolist()
        assert rn.is_between_form(ts, ns)
        (te, ne), (ts, ns) = rn.expect_bounds(row, *W["block_end"]).tolist()
        assert rn.is_between_form(te, ne)
        (te, ne), (ts, ns) = rn.expect_bounds(row, *W["real_key_at_T"]).tolist()
        assert te == ts and rn.is_between_form(ts, ns) and ne > 0                   # one threshold, mixed forms
        assert (rn.score_keys(row) == (ts & 0xffffffff)).sum() > ne                 # ... which is a real key
        (te, ne), (ts, ns) = rn.expect_bounds(row, *W["two_blocks"]).tolist()
        keys = rn.score_keys(row)
        assert ne > 0 and ns > 0 and not ((keys > (te & 0xffffffff)) & (keys < (ts & 0xffffffff))).any()    # W == 0, both tails
        (te, ne), (ts, ns) = rn.expect_bounds(row, *W["three_blocks"]).tolist()
        assert ((keys > (te & 0xffffffff)) & (keys < (ts & 0xffffffff))).any()


def test_expect_window_counts_and_padding():
    row = np.array([1.0, -np.inf, 3.0, np.nan, 3.0, -0.0], np.float32)
    order = rn.full_order(row)
    assert order.tolist() == [2, 4, 0, 5]
    ids, vals, count, total = rn.expect_window(row, order, 1, 2)
    assert (count, total) == (2, 4) and ids[:2].tolist() == [4, 0] and (ids[2:] == -1).all() and np.isneginf(vals[2:]).all()
    ids, vals, count, total = rn.expect_window(row, order, 3, 1024)
    assert count == 1 and vals[0].tobytes() == np.float32(0.0).tobytes()            # -0.0 comes back as +0.0
    assert rn.expect_window(row, order, 2 ** 40, 5)[2] == 0
