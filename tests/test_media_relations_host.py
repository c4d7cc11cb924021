"""CPU: recommendersystem_amd/relations.py (Training/media_relations.jl, pairwise_dataset.jl's smoothed_wilson_score) against the literal
restatement in tests/_media_relations_np.py.  No GPU: the watch-order counts are read through a dense numpy stand-in."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _media_relations_np as ref  # noqa: E402

from recommendersystem_amd import relations as rel  # noqa: E402
from recommendersystem_amd.model import csc_parts  # noqa: E402


def dense(a):
    return rel.csc_dense(a)


def details_of(media_rows):
    return {(r["medium"], r["matchedid"]): r["mediatype"] for r in media_rows}


def test_reclassification():
    media = [{"medium": 0, "matchedid": i, "mediatype": t, "source": "mal", "count": 1, "startdate": None}
             for i, t in enumerate(["Manga", "Light Novel", "Novel", "Manhwa", "One-shot", "Doujinshi"])]
    media += [{"medium": 1, "matchedid": i, "mediatype": "TV", "source": "mal", "count": 1, "startdate": None} for i in range(3)]
    rows = [(0, 0, 0, 1, "unknown"),      # manga -> light novel: adaptation
            (0, 2, 0, 3, "unknown"),      # novel -> manhwa: adaptation
            (0, 0, 0, 3, "unknown"),      # manga -> manhwa: stays
            (0, 1, 0, 2, "unknown"),      # novel -> novel: stays
            (0, 4, 1, 2, "unknown"),      # cross-medium: adaptation
            (1, 0, 1, 1, "unknown"),      # TV -> TV: stays
            (0, 0, 0, 1, "sequel"),       # not unknown: untouched
            (0, 5, 0, 1, "unknown")]      # doujinshi -> light novel: adaptation
    rows = [dict(zip(("source_medium", "source_matchedid", "target_medium", "target_matchedid", "relation"), r)) for r in rows]
    want = [r["relation"] for r in ref.get_media_relations(rows, details_of(media))]
    assert want == ["adaptation", "adaptation", "unknown", "unknown", "adaptation", "unknown", "sequel", "adaptation"]
    details = rel.get_media_details({0: ref.media_columns(media[:6]), 1: ref.media_columns(media[6:])})
    got = rel.get_media_relations(ref.relation_columns(rows), details)["relation"]
    assert got == want
    bad = [dict(rows[2], target_matchedid=9)]
    with pytest.raises(ValueError):
        rel.get_media_relations(ref.relation_columns(bad), details)


def random_graph(rng, V, n_edges, big_component=0):
    rows = []
    for _ in range(n_edges):
        rows.append((int(rng.integers(0, V)), int(rng.integers(0, V))))
    for k in range(big_component - 1):                  # a chain through ids 0 .. big_component - 1, closed into one cycle
        rows.append((k, k + 1))
    if big_component:
        rows.append((big_component - 1, 0))
    rows += [(i, i) for i in rng.integers(0, V, 3)]      # self-loops
    kinds = ["sequel", "other", "summary"]
    return [{"source_medium": 0, "source_matchedid": a, "target_medium": 0, "target_matchedid": b,
             "relation": kinds[rng.integers(0, len(kinds))]} for a, b in rows]


@pytest.mark.parametrize("V,n_edges,big", [(80, 120, 0), (200, 150, 0), (2300, 400, 2000)])
@pytest.mark.parametrize("symmetric", [False, True])
def test_symmetric_transitive_matrices(V, n_edges, big, symmetric):
    rng = np.random.default_rng(V + n_edges + symmetric)
    rows = random_graph(rng, V, n_edges, big)
    cols = ref.relation_columns(rows)
    kinds = ["sequel", "other"]
    for transitive in (False, True):
        want = ref.get_matrix(rows, 0, kinds, V, symmetric=symmetric, transitive=transitive)
        got = rel.get_matrix(cols, 0, kinds, V, symmetric=symmetric, transitive=transitive)
        np.testing.assert_array_equal(dense(got), want)
        assert (got[2] == 1).all() and (np.diff(got[0]) >= 0).all()
    # transitive_closure on its own keeps the diagonal of nodes on cycles
    S = rel.get_relations(cols, 0, 0, kinds, (V, V))
    np.testing.assert_array_equal(dense(rel.transitive_closure(S)), ref.transitive_closure(ref.get_relations(rows, 0, 0, kinds, (V, V))))


def test_transitive_edge_removal_is_sequential():
    # edges (0,2), (0,1), (1,2), (0,3), (3,1): column-major order meets (0,1) first, which (0,3)+(3,1) removes; (0,2) then has no
    # witness left (its witness was 1 through (0,1)), so it stays -- a simultaneous removal would drop it too
    M = np.zeros((4, 4), np.float32)
    for i, j in [(0, 2), (0, 1), (1, 2), (0, 3), (3, 1)]:
        M[i, j] = 1
    want = ref.remove_transitive_edges(M)
    assert want[0, 2] == 1 and want[0, 1] == 0
    simultaneous = M.copy()
    simultaneous[(M @ M > 0) & (M > 0)] = 0
    assert not (simultaneous == want).all()
    i, j = np.nonzero(M.T)
    got = rel.remove_transitive_edges(j.astype(np.int64), i.astype(np.int64), (4, 4))
    np.testing.assert_array_equal(dense(got), want)
    rng = np.random.default_rng(3)
    for _ in range(5):
        M = (rng.random((40, 40)) < 0.12).astype(np.float32)
        np.fill_diagonal(M, 0)
        r, c = np.nonzero(M)
        np.testing.assert_array_equal(dense(rel.remove_transitive_edges(r, c, (40, 40))), ref.remove_transitive_edges(M))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_dependencies_against_restatement(seed):
    rng = np.random.default_rng(seed)
    V0, V1 = 40, 30
    media_rows = ref.synthetic_media(rng, 0, V0)
    relrows = ref.synthetic_relations(rng, V0, V1, 220)
    relrows = ref.get_media_relations(relrows, {**details_of(media_rows), **details_of(ref.synthetic_media(rng, 1, V1))})
    W = rng.integers(0, 5, (V0, V0)).astype(np.int32)
    W[rng.random((V0, V0)) < 0.3] = 0
    want = ref.save_dependencies(relrows, media_rows, 0, V0, W)
    got = rel.save_dependencies(ref.relation_columns(relrows), ref.media_columns(media_rows), 0, V0, ref.DenseWatches(W))
    np.testing.assert_array_equal(dense(got), want)
    assert want.sum() > 0
    np.testing.assert_array_equal(dense(rel.save_related(ref.relation_columns(relrows), 0, V0)), ref.save_related(relrows, 0, V0))
    np.testing.assert_array_equal(dense(rel.save_recaps(ref.relation_columns(relrows), 0, V0)), ref.save_recaps(relrows, 0, V0))
    np.testing.assert_array_equal(dense(rel.save_adaptations(ref.relation_columns(relrows), 0, V0, V1)), ref.save_adaptations(relrows, 0, V0, V1))
    np.testing.assert_array_equal(dense(rel.save_adaptations(ref.relation_columns(relrows), 1, V1, V0)), ref.save_adaptations(relrows, 1, V1, V0))


def test_dependencies_missing_popularity_raises():
    rng = np.random.default_rng(5)
    media_rows = ref.synthetic_media(rng, 0, 10, missing={3})
    relrows = [{"source_medium": 0, "source_matchedid": 3, "target_medium": 0, "target_matchedid": 4, "relation": "sequel"}]
    W = np.ones((10, 10), np.int32)
    with pytest.raises(ValueError):
        ref.save_dependencies(relrows, media_rows, 0, 10, W)
    with pytest.raises(ValueError):
        rel.save_dependencies(ref.relation_columns(relrows), ref.media_columns(media_rows), 0, 10, ref.DenseWatches(W))


def test_popularity_ties_and_sources():
    rows = [{"medium": 0, "matchedid": i, "mediatype": "Manga", "source": s, "count": c, "startdate": None}
            for i, s, c in [(0, "mal", 3), (0, "mal", 5), (0, "anilist", 2), (1, "mal", 7), (2, "kitsu", 4), (2, "kitsu", 1), (2, "mal", 3),
                            (3, "mal", 0)]]
    cols = ref.media_columns(rows)
    for a in range(4):
        for b in range(4):
            assert rel.is_more_popular(cols, 0.5, a, b) == ref.is_more_popular(rows, 0.5, a, b), (a, b)
    assert not rel.is_more_popular(cols, 0.5, 0, 1) and not rel.is_more_popular(cols, 0.5, 1, 0)    # 7 == 7: a tie is not "more"
    with pytest.raises(ValueError):
        rel.is_more_popular(dict(cols, matchedid=np.array([0, 0, 0, 1, 2, 2, 2, 5])), 0.5, 3, 0)


def test_released_after_dates():
    dates = {0: "2001-10", 1: "2001-9", 2: "2001", 3: None, 4: "2001-10-03", 5: "2002-01-01", 6: "2001-10-3"}
    rows = [{"medium": 0, "matchedid": i, "mediatype": "TV", "source": "mal", "count": 1, "startdate": d} for i, d in dates.items()]
    rows.append({"medium": 0, "matchedid": 0, "mediatype": "TV", "source": "kitsu", "count": 1, "startdate": "1990"})   # first row wins
    cols = ref.media_columns(rows)
    for a in range(8):
        for b in range(8):
            want = ref.is_released_after(rows, a, b)
            assert rel.is_released_after(cols, a, b, rel.startdates(cols, 8)) == want, (a, b)
    assert not rel.is_released_after(cols, 0, 1)          # "10" < "9" as strings
    assert rel.is_released_after(cols, 1, 0)
    assert not rel.is_released_after(cols, 2, 4) and not rel.is_released_after(cols, 4, 2)    # equal leading fields
    assert not rel.is_released_after(cols, 3, 0) and not rel.is_released_after(cols, 0, 3)    # missing date
    assert not rel.is_released_after(cols, 7, 0)          # no row at all
    assert rel.is_released_after(cols, 6, 4)              # "3" > "03"


def item(m, i, s):
    return {"medium": m, "matchedid": i, "status": s}


def test_project_earliest_cases():
    user = {"items": [item(0, 5, 3), item(0, 7, 0), item(1, 5, 7), item(0, 5, 6), item(0, 7, 8), item(0, 9, 5), item(0, 2, 9),
                      item(0, 9, 6), item(0, 5, 0), item(1, 2, 0)]}
    want = ref.project_earliest(user, 0)
    assert want == [7, 5, 2, 9]          # 5 unwatched first (status 3), watched later; 7 at status 0; medium 1 skipped; repeats dropped
    assert rel.project_earliest(user, 0) == want
    assert rel.project_earliest(user, 1) == ref.project_earliest(user, 1) == [5, 2]


def random_users(rng, n, V0, V1, max_len=40):
    users = []
    for _ in range(n):
        L = int(rng.integers(0, max_len))
        users.append({"items": [item(int(rng.integers(0, 2)), int(rng.integers(0, V0)), int(rng.integers(0, 10))) for _ in range(L)]})
    return users


def test_project_earliest_csr_matches_per_user():
    rng = np.random.default_rng(11)
    users = random_users(rng, 300, 50, 30) + [{"items": []}]
    for m in (0, 1):
        off, items = rel.project_earliest_csr(users, m)
        assert off.dtype == np.int64 and items.dtype == np.int32 and off.size == len(users) + 1
        for u, user in enumerate(users):
            assert items[off[u]:off[u + 1]].tolist() == ref.project_earliest(user, m)
    off, items = rel.project_earliest_csr([{"items": [item(1, 3, 0)]}], 0)
    assert off.tolist() == [0, 0] and items.size == 0


def test_watch_counts_gather_and_literal_loops():
    rng = np.random.default_rng(4)
    users = random_users(rng, 200, 30, 20)
    hist = [ref.project_earliest(u, 0) for u in users]
    W, n = ref.get_watch_order(hist, 30)
    W2, n2 = ref.get_watch_order_fast(hist, 30)
    np.testing.assert_array_equal(W, W2)
    assert n == n2 == sum(1 for h in hist if h)
    r, c = np.nonzero(W)
    indptr = np.zeros(31, np.int64)
    np.cumsum(np.bincount(r, minlength=30), out=indptr[1:])
    wc = rel.WatchCounts(indptr, c, W[r, c], (30, 30))
    np.testing.assert_array_equal(wc.toarray(), W)
    a, b = rng.integers(0, 30, 500), rng.integers(0, 30, 500)
    np.testing.assert_array_equal(wc.gather(a, b), W[a, b])
    for x, y in zip(a[:50], b[:50]):
        assert rel.is_watched_before(wc, 0.5, int(x), int(y)) == ref.is_watched_before(W, 0.5, x, y)


def test_pair_score_formula_edges():
    cases = [(5, 3, 0),        # k > n: k = min(n, k) -> p = 1
             (0, 10, 0),       # p = 0: the lower bound clamps at 0, then eps(Float32)
             (1, 10, 0),       # p - z sd < 0: clamp
             (9, 10, 0), (40, 50, 100), (3, 4, 18), (3, 4, 38), (3, 4, 28), (3, 4, 48),   # 0.5 and 1.5 and 2.5: half to even
             (2, 0, 0),        # n == 0 and no smoothing: NaN
             (2, 0, 10),       # n == 0 smoothed to round(0.5) = 0: NaN
             (2, 0, 30)]       # n == 0 smoothed to round(1.5) = 2: k = min(0, 2) = 0
    k, n, w = (np.asarray(x) for x in zip(*cases))
    got = rel.smoothed_wilson_score(k, n, w)
    for (kk, nn, ww), g in zip(cases, got):
        want = ref.smoothed_wilson_score(kk, nn, ww)
        if math.isnan(want):
            assert math.isnan(g), (kk, nn, ww)
        else:
            assert g == want, (kk, nn, ww, g, want)
    assert got[1] == np.finfo(np.float32).eps and got[2] == np.finfo(np.float32).eps
    assert np.isnan(got[9]) and np.isnan(got[10]) and got[11] == np.finfo(np.float32).eps
    # round half to even: w - 2n = 10 -> 0.5 -> 0, 30 -> 1.5 -> 2, 50 -> 2.5 -> 2
    assert rel.smoothed_wilson_score(3, 4, 18) == ref.smoothed_wilson_score(3, 4, 4 * 2 + 10)
    assert rel.smoothed_wilson_score(3, 4, 48) == ref.smoothed_wilson_score(3, 6, 0)


def test_pair_scores_gathers_both_directions():
    rng = np.random.default_rng(8)
    W = rng.integers(0, 20, (25, 25)).astype(np.int32)
    s, t = rng.integers(0, 25, 300), rng.integers(0, 25, 300)
    count = rng.integers(0, 30, 300)
    pop = rng.integers(0, 400, 300)
    score, watches = rel.pair_scores(ref.DenseWatches(W), s, t, count, pop)
    np.testing.assert_array_equal(watches, W[s, t].astype(np.int64) + W[t, s])
    for q in range(300):
        want = ref.smoothed_wilson_score(int(count[q]), int(W[s[q], t[q]] + W[t[q], s[q]]), int(pop[q]))
        assert (math.isnan(want) and math.isnan(score[q])) or score[q] == want


def test_tuples_accepted_by_csc_parts():
    rng = np.random.default_rng(9)
    relrows = ref.synthetic_relations(rng, 30, 20, 150)
    cols = ref.relation_columns(relrows)
    for a in (rel.save_related(cols, 0, 30), rel.save_recaps(cols, 1, 20), rel.save_adaptations(cols, 0, 30, 20),
              rel.get_matrix(cols, 0, [], 30)):
        indptr, indices, data, shape = csc_parts(a)
        assert indptr.size == shape[1] + 1 and indices.size == data.size == indptr[-1]
        assert (data == 1).all()
    assert csc_parts(rel.get_matrix(cols, 0, [], 30))[0][-1] == 0


def test_npz_round_trip(tmp_path):
    rng = np.random.default_rng(12)
    relrows = ref.synthetic_relations(rng, 30, 20, 150)
    cols = ref.relation_columns(relrows)
    d = {}
    for kind, a in (("dependencies", rel.get_matrix(cols, 0, ["sequel"], 30)), ("related", rel.save_related(cols, 0, 30)),
                    ("recaps", rel.save_recaps(cols, 0, 30)), ("adaptations", rel.save_adaptations(cols, 0, 30, 20))):
        rel._save_csc(d, f"0.{kind}", a)
    np.savez(os.path.join(tmp_path, "media_relations.0.npz"), **d)
    out = rel.load_relations(str(tmp_path))
    assert sorted(out) == ["0.adaptations", "0.dependencies", "0.recaps", "0.related"]
    np.testing.assert_array_equal(dense(out["0.related"]), dense(rel.save_related(cols, 0, 30)))
    assert out["0.adaptations"][3] == (30, 20)
