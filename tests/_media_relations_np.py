"""Literal restatement of Training/media_relations.jl and of pairwise_dataset.jl's smoothed_wilson_score on dense numpy arrays and
plain loops: the test-side reference of recommendersystem_amd/relations.py and of the rsys_watch_order_* kernels.  Ids are 0-based;
matrices are dense, indexed [row, col] as the Julia matrices are (shifted by one)."""
import math

import numpy as np

MANGA_TYPES = {"Manhwa", "Manhua", "Manga", "OEL", "Doujinshi", "One-shot"}
NOVEL_TYPES = {"Light Novel", "Novel"}


def get_media_relations(rows, details):
    """rows: list of dicts source_medium, source_matchedid, target_medium, target_matchedid, relation; details {(m, id): mediatype}"""
    out = []
    for r in rows:
        r = dict(r)
        if r["relation"] == "unknown":
            m1, id1, m2, id2 = r["source_medium"], r["source_matchedid"], r["target_medium"], r["target_matchedid"]
            if m1 != m2:
                r["relation"] = "adaptation"
            else:
                d1, d2 = details[(m1, id1)], details[(m2, id2)]
                if d1 in MANGA_TYPES and d2 in NOVEL_TYPES or d1 in NOVEL_TYPES and d2 in MANGA_TYPES:
                    r["relation"] = "adaptation"
        out.append(r)
    return out


def get_relations(rows, source_medium, target_medium, relations, shape):
    M = np.zeros(shape, np.float32)
    for r in rows:
        if r["source_medium"] == source_medium and r["target_medium"] == target_medium and r["relation"] in relations:
            M[r["source_matchedid"], r["target_matchedid"]] += 1.0
    M[M > 0] = 1
    return M


def transitive_closure(S):
    closure = S.astype(bool)
    for _ in range(S.shape[0]):
        c = closure.astype(np.float32)
        new_closure = closure | ((c @ c) > 0)
        if (new_closure == closure).all():
            break
        closure = new_closure
    return closure.astype(S.dtype)


def get_matrix(rows, medium, relations, V, symmetric=False, transitive=False):
    S = get_relations(rows, medium, medium, relations, (V, V))
    if symmetric:
        S = np.maximum(S, S.T)
    if transitive:
        S = transitive_closure(S)
    for i in range(V):
        S[i, i] = 0
    return S


def get_popularity(media_rows, itemid):
    source_to_count = {}
    for r in media_rows:
        if r["matchedid"] == itemid:
            source_to_count[r["source"]] = max(source_to_count.get(r["source"], 0), r["count"])
    if not source_to_count:
        raise ValueError("sum over an empty collection")
    return sum(source_to_count.values())


def is_more_popular(media_rows, cutoff, a1, a2):
    return get_popularity(media_rows, a1) > (get_popularity(media_rows, a1) + get_popularity(media_rows, a2)) * cutoff


def is_released_after(media_rows, a1, a2):
    def get_startdate(itemid):
        for r in media_rows:
            if r["matchedid"] == itemid:
                return r["startdate"]
        return None
    s1, s2 = get_startdate(a1), get_startdate(a2)
    if s1 is None or s2 is None:
        return False
    f1, f2 = s1.split("-"), s2.split("-")
    for k in range(min(len(f1), len(f2))):
        if f1[k] > f2[k]:
            return True
        if f1[k] < f2[k]:
            return False
    return False


def project_earliest(user, medium):
    watching_status = 6
    seen, items = set(), []
    for x in user["items"]:
        if x["medium"] != medium or x["matchedid"] in seen:
            continue
        watched = x["status"] == 0 or x["status"] >= watching_status
        if not watched:
            continue
        seen.add(x["matchedid"])
        items.append(x["matchedid"])
    return items


def get_watch_order(histories, V):
    """the loops of get_watch_order (:184-193) over projected histories: (W int32 [V][V], num_users)"""
    W = np.zeros((V, V), np.int32)
    num_users = 0
    for h in histories:
        if len(h) > 0:
            num_users += 1
        for i in range(len(h)):
            for j in range(i + 1, len(h)):
                W[h[i], h[j]] += 1
    return W, num_users


def get_watch_order_fast(histories, V):
    """the same sums with one numpy update per row (for histories too long for the literal loops)"""
    W = np.zeros((V, V), np.int32)
    num_users = 0
    for h in histories:
        h = np.asarray(h, np.int64)
        num_users += h.size > 0
        for i in range(h.size - 1):
            W[h[i], h[i + 1:]] += 1
    return W, num_users


def is_watched_before(W, cutoff, a1, a2):
    return W[a1, a2] > cutoff * (W[a1, a2] + W[a2, a1])


def save_dependencies(rows, media_rows, medium, V, W):
    R = sum(get_matrix(rows, medium, [x], V, transitive=True) for x in ["sequel", "prequel", "parent_story", "side_story"])
    R = R + R.T
    M = np.zeros((V, V), np.float32)
    nz = [(i, j, R[i, j]) for j in range(V) for i in range(V) if R[i, j] != 0]     # findnz: column-major
    for i, j, v in nz:
        if v == 0:
            continue
        if is_more_popular(media_rows, 0.5, j, i) and is_watched_before(W, 0.5, j, i) and not is_released_after(media_rows, j, i):
            M[i, j] = 1
    return remove_transitive_edges(M)


def remove_transitive_edges(M):
    """the second loop of save_dependencies (:240-248), in place on a copy"""
    M = M.copy()
    V = M.shape[0]
    nz = [(i, j) for j in range(V) for i in range(V) if M[i, j] != 0]
    for i, j in nz:
        for k in range(V):
            if M[i, j] > 0 and M[i, k] > 0 and M[k, j] > 0:
                M[i, j] = 0
    return M


def save_related(rows, medium, V):
    rel = {"sequel", "prequel", "parent_story", "side_story", "alternative_version", "summary", "full_story", "adaptation",
           "alternative_setting", "spin_off", "compilation", "contains", "other"}
    return get_matrix(rows, medium, rel, V, symmetric=True, transitive=True)


def save_recaps(rows, medium, V):
    return get_matrix(rows, medium, {"alternative_version", "summary", "full_story", "adaptation", "contains", "compilation"}, V, symmetric=True)


def save_adaptations(rows, medium, V, V_other):
    return get_relations(rows, medium, 1 - medium, {"adaptation", "source", "alternative_version", "parent_story", "side_story"}, (V, V_other))


def smoothed_wilson_score(k, n, w):
    k = min(n, k)
    n = n + int(round(max(w - 2 * n, 0) * 0.05))          # Python's round is half-even, as Julia's
    if n == 0:
        return float("nan")
    p = k / n
    lower = max(p - 1.959963984540054 * math.sqrt(p * (1 - p) / n), 0.0)
    return max(lower, float(np.finfo(np.float32).eps))


# ---------------------------------------------------------------- synthetic inputs shared by the CPU and GPU tests
RELATION_KINDS = ["sequel", "prequel", "parent_story", "side_story", "alternative_version", "summary", "full_story", "adaptation",
                  "alternative_setting", "spin_off", "compilation", "contains", "other", "source", "character", "unknown"]
MEDIATYPES = ["Manga", "Manhwa", "Light Novel", "Novel", "One-shot", "TV", "Movie", "OVA"]


def synthetic_media(rng, medium, V, dup_sources=True, missing=()):
    """media rows of one medium: every id but those in `missing` has 1-3 rows (sources), counts with ties, dates full, partial or empty"""
    rows = []
    for i in range(V):
        if i in missing:
            continue
        for s in (["mal", "anilist", "kitsu"][:rng.integers(1, 4)] if dup_sources else ["mal"]):
            for _ in range(rng.integers(1, 3)):
                y, mo, d = rng.integers(1995, 2003), rng.integers(1, 13), rng.integers(1, 29)
                date = [f"{y}-{mo}-{d}", f"{y}-{mo}", f"{y}", ""][rng.integers(0, 4)]
                rows.append({"medium": medium, "matchedid": i, "mediatype": MEDIATYPES[rng.integers(0, len(MEDIATYPES))], "source": s,
                             "count": int(rng.integers(0, 6)), "startdate": date or None})
    return rows


def synthetic_relations(rng, V0, V1, n):
    rows = []
    for _ in range(n):
        m1, m2 = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        if rng.random() < 0.7:
            m2 = m1
        rows.append({"source_medium": m1, "source_matchedid": int(rng.integers(0, V0 if m1 == 0 else V1)), "target_medium": m2,
                     "target_matchedid": int(rng.integers(0, V0 if m2 == 0 else V1)),
                     "relation": RELATION_KINDS[rng.integers(0, len(RELATION_KINDS))]})
    return rows


def media_columns(rows):
    """rows -> the columns relations.read_media returns"""
    return {"medium": np.asarray([r["medium"] for r in rows], np.int64), "matchedid": np.asarray([r["matchedid"] for r in rows], np.int64),
            "count": np.asarray([r["count"] for r in rows], np.int64), "mediatype": [r["mediatype"] for r in rows],
            "source": [r["source"] for r in rows], "startdate": [r["startdate"] for r in rows]}


def relation_columns(rows):
    out = {k: np.asarray([r[k] for r in rows], np.int64) for k in ("source_medium", "source_matchedid", "target_medium", "target_matchedid")}
    out["relation"] = [r["relation"] for r in rows]
    return out


class DenseWatches:
    """a dense numpy W with the gather the host functions read through"""

    def __init__(self, W):
        self.W = W

    def gather(self, a, b):
        return self.W[np.asarray(a, np.int64), np.asarray(b, np.int64)]
