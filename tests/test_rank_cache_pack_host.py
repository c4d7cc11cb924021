"""CPU: serve.rank_cache_pack_plan, the packed ranking plan as data, against a brute-force restatement of its properties --
every user stored once, every candidate ranked once, segments on tile boundaries, inside their rows and disjoint, waves within the slots,
and the rule that picks between the packed layout and one segment per row -- and serve.render_full_forwards(pack_store=True), the
render pipeline's packed store forwards as data."""
import itertools

import numpy as np
import pytest

from recommendersystem_amd import serve


def _tokens(forwards):
    return sum(row_len * (1 + max(p[1] for p in placed)) for row_len, placed in forwards)


def _single(lengths, S, max_rows):
    """one segment per row at the trim length, restated: (forwards, tokens)"""
    groups = [lengths[i:i + max_rows] for i in range(0, len(lengths), max_rows)]
    return len(groups), sum(len(g) * serve.trim_length(max(g), S) for g in groups)


def _check_stage(forwards, S, max_rows, length_of):
    """segments 32-aligned, inside a row, no tile twice; rows 0 .. n - 1 with n <= max_rows; row_len = trim_length of the fullest row"""
    for row_len, placed in forwards:
        rows = sorted({p[1] for p in placed})
        assert rows == list(range(len(rows))) and len(rows) <= max_rows
        taken = set()
        ends = []
        for p in placed:
            row, c0, n = p[1], p[2], length_of(p)
            assert c0 % 32 == 0 and n >= 1 and c0 + n <= min(row_len, S)
            tiles = {(row, t) for t in range(c0 // 32, -(-(c0 + n) // 32))}
            assert not tiles & taken
            taken |= tiles
            ends.append(c0 + n)
        assert row_len == serve.trim_length(max(ends), S)


def _check_plan(n_hist, n_cand, S, max_rows, slots):
    plan = serve.rank_cache_pack_plan(n_hist, n_cand, S, max_rows, slots)
    stored, ranked = [], []
    at = 0
    for stores, cands in plan:
        users = sorted(p[0] for _, placed in stores for p in placed)
        assert users == list(range(at, at + len(users))) and 1 <= len(users) <= slots          # waves in user order, within the slots
        assert len(users) == slots or at + len(users) == len(n_hist)
        _check_stage(stores, S, max_rows, lambda p: p[3])
        _check_stage(cands, S, max_rows, lambda p: p[4])
        slot_of = {}
        for _, placed in stores:
            for u, _, _, nh, slot in placed:
                assert nh == n_hist[u] and slot == u - at and u not in slot_of
                slot_of[u] = slot
                stored.append(u)
        for _, placed in cands:
            for u, _, _, first, n, slot in placed:
                assert slot == slot_of[u] and 1 <= n <= S                                      # a candidate chunk reads its own wave's slot
                ranked += [(u, first + j) for j in range(n)]
        # the choice rule, per stage and wave: never more forwards than one segment per row; with as many, never more tokens
        hl = [n_hist[u] for u in users]
        cl = [min(S, n_cand[u] - c) for u in users for c in range(0, n_cand[u], S)]
        for forwards, lengths in ((stores, hl), (cands, cl)):
            if not lengths:
                assert forwards == []
                continue
            nf, nt = _single(lengths, S, max_rows)
            assert len(forwards) <= nf and (len(forwards) < nf or _tokens(forwards) <= nt)
            if not (len(forwards) < nf or _tokens(forwards) < nt):          # nothing saved: one segment per row, at column 0, in order
                assert (len(forwards), _tokens(forwards)) == (nf, nt)
                assert [(p[1], p[2]) for _, placed in forwards for p in placed] == [(i % max_rows, 0) for i in range(len(lengths))]
        at += len(users)
    assert sorted(stored) == list(range(len(n_hist)))
    assert sorted(ranked) == [(u, j) for u in range(len(n_hist)) for j in range(n_cand[u])]
    return plan


def test_random_plans_hold_the_properties():
    rng = np.random.default_rng(3)
    for S, max_rows, slots in itertools.product((64, 128, 256), (1, 2, 4), (1, 4, 16)):
        for _ in range(6):
            n = int(rng.integers(1, 24))
            n_hist = [int(x) for x in rng.integers(1, S + 1, size=n)]
            if rng.random() < 0.5:
                n_hist = [max(1, h // 8) for h in n_hist]
            n_cand = [int(x) for x in rng.integers(0, 2 * S + 8, size=n)]
            if rng.random() < 0.5:
                n_cand = [c % 7 for c in n_cand]
            _check_plan(n_hist, n_cand, S, max_rows, slots)


def test_four_users_of_75_events_stay_one_per_row():
    """S = 256, max_rows 4: packed is 2 rows x 192 columns, one per row is 4 x 96 -- one forward and 384 columns either way, so the
    stage stays one segment per row (the plan of 4zb that ran 1.5 x the tokens must not come back: 3 x 300-event users per 1024-column row)"""
    (stores, _), = _check_plan([75] * 4, [1] * 4, 256, 4, 16)
    assert stores == [(96, [(u, u, 0, 75, u) for u in range(4)])]
    (stores, _), = _check_plan([300] * 4, [1] * 4, 1024, 4, 16)
    assert stores == [(320, [(u, u, 0, 300, u) for u in range(4)])]


def test_nine_users_of_4_events_share_rows():
    """one forward instead of three; at S = 128 a row has four tiles, so nine segments take three rows; from S = 288 on they are one row"""
    (stores, cands), = _check_plan([4] * 9, [2] * 9, 128, 4, 16)
    assert len(stores) == 1 and len(cands) == 1
    assert [(p[1], p[2]) for p in stores[0][1]] == [(u // 4, 32 * (u % 4)) for u in range(9)]
    (stores, cands), = _check_plan([4] * 9, [2] * 9, 512, 4, 16)
    assert stores == [(288, [(u, 0, 32 * u, 4, u) for u in range(9)])]
    assert cands == [(288, [(u, 0, 32 * u, 0, 2, u) for u in range(9)])]
    # with four slots the same users are three waves
    assert [len(w[0][0][1]) for w in _check_plan([4] * 9, [2] * 9, 512, 4, 4)] == [4, 4, 1]


def test_a_tail_segment_packs_beside_another_users():
    S = 128
    (_, cands), = _check_plan([10, 20], [S + 5, 3], S, 4, 16)
    assert len(cands) == 1
    placed = cands[0][1]
    assert (0, 0, 0, 0, S, 0) in placed
    tail = next(p for p in placed if p[0] == 0 and p[3] == S)
    other = next(p for p in placed if p[0] == 1)
    assert tail[4] == 5 and other[4] == 3 and tail[1] == other[1] and tail[2] != other[2]     # one row, different tiles


def test_bad_arguments():
    for args in (([0], [1], 128, 4, 4), ([129], [1], 128, 4, 4), ([1], [-1], 128, 4, 4), ([1], [1], 128, 4, 0), ([1, 2], [1], 128, 4, 4)):
        with pytest.raises(ValueError):
            serve.rank_cache_pack_plan(*args)


def test_render_full_forwards_with_packed_store_rows():
    """(store, candidate, empty-history) forwards of the pipeline under rsys_serving_pack_ranking_set on the three cases above, beside the
    unpacked counts; the store stage is rank_cache_pack_plan's"""
    S = 128
    cases = [([75] * 4, [1] * 4, 256, 4, 16, (1, 1, 0), (1, 1, 0)),            # one per row either way
             ([4] * 9, [2] * 9, 128, 4, 16, (3, 3, 0), (1, 3, 0)),              # three store forwards -> one
             ([4] * 9, [2] * 9, 128, 4, 4, (3, 3, 0), (3, 3, 0)),               # four slots: three waves, nothing to gain
             ([10, 20], [S + 5, 3], S, 4, 16, (1, 1, 0), (1, 1, 0)),            # (the pipeline's candidate rows stay one chunk per row)
             ([10, 0, 20, 0], [S + 5, 70, 3, 5], S, 4, 16, (1, 1, 1), (1, 1, 1)),
             ([300] * 15, [20] * 15, 1024, 4, 16, (4, 4, 0), (2, 4, 0))]       # DESIGN 4w's case (c): 4 of 12 forwards -> 2
    for n_hist, n_cand, s, max_rows, slots, unpacked, packed in cases:
        assert serve.render_full_forwards(n_hist, n_cand, s, max_rows) == unpacked
        got = serve.render_full_forwards(n_hist, n_cand, s, max_rows, pack_store=True, slots=slots)
        assert got == packed, (n_hist, n_cand, got)
        hist = [(h, c) for h, c in zip(n_hist, n_cand) if h >= 1]
        plan = serve.rank_cache_pack_plan([h for h, _ in hist], [c for _, c in hist], s, max_rows, slots)
        assert got[0] == sum(len(stores) for stores, _ in plan)
        rows = serve.render_full_store_rows(n_hist, s, max_rows, slots)
        assert rows == [(1 + max(p[1] for p in placed), row_len) for stores, _ in plan for row_len, placed in stores]
    assert serve.render_full_forwards([4] * 9, [2] * 9, 128, 4, pack_store=True) == (3, 3, 0)      # slots default to max_rows
