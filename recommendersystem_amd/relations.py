"""The media relation tables and the watch-order matrix (Training/media_relations.jl) under the reference's names.

`get_watch_order` counts, for every ordered pair of items of one medium, the training users who watched the first before the second.
The counting runs on the device through the rsys_watch_order_* entry points of include/rsys.h (`WatchOrder`); this module holds the
projection of the user lists, the relation matrices, the dependency rule that reads the counts, the pair scores of
item_similarity/pairwise_dataset.jl and the .npz files.  Sparse matrices are 0-based CSC `(indptr, indices, data float32, shape)`
tuples, the form `model.csc_parts` and `serve.julia_csc` take.  Inputs are the reference's files ({manga,anime}.csv,
media_relations.csv, users/training/*/*.msgpack, read with the stdlib csv module and msgpack) or the same columns passed as arrays.
Deviations: a missing (medium, matchedid) detail raises ValueError where Julia throws KeyError; the files are .npz, not JLD2, and
nothing is uploaded."""
import csv
import ctypes as C
import glob
import os

import numpy as np

from ._lib import check, lib

MEDIA = {0: "manga", 1: "anime"}
MANGA_TYPES = frozenset(["Manhwa", "Manhua", "Manga", "OEL", "Doujinshi", "One-shot"])
NOVEL_TYPES = frozenset(["Light Novel", "Novel"])
WATCHING_STATUS = 6
DEPENDENCY_RELATIONS = ("sequel", "prequel", "parent_story", "side_story")
RELATED_RELATIONS = frozenset(["sequel", "prequel", "parent_story", "side_story", "alternative_version", "summary", "full_story", "adaptation",
                               "alternative_setting", "spin_off", "compilation", "contains", "other"])
RECAP_RELATIONS = frozenset(["alternative_version", "summary", "full_story", "adaptation", "contains", "compilation"])
ADAPTATION_RELATIONS = frozenset(["adaptation", "source", "alternative_version", "parent_story", "side_story"])
WILSON_Z = 1.959963984540054             # quantile(Normal(), 1 - 0.05 / 2)
EPS_F32 = float(np.finfo(np.float32).eps)


# ---------------------------------------------------------------- inputs
def read_media(datadir, medium):
    """{manga,anime}.csv as columns: medium, matchedid, count (int64 arrays), mediatype, source (str lists), startdate (str or None)"""
    cols = {k: [] for k in ("medium", "matchedid", "mediatype", "source", "count", "startdate")}
    with open(os.path.join(datadir, f"{MEDIA[medium]}.csv"), newline="") as f:
        for row in csv.DictReader(f):
            for k in cols:
                cols[k].append(row.get(k))
    out = {k: np.asarray([int(x) for x in cols[k]], np.int64) for k in ("medium", "matchedid", "count")}
    out["mediatype"] = list(cols["mediatype"])
    out["source"] = list(cols["source"])
    out["startdate"] = [x if x not in (None, "") else None for x in cols["startdate"]]
    return out


def read_media_relations(datadir):
    """media_relations.csv as columns: source_medium, source_matchedid, target_medium, target_matchedid (int64), relation (str list)"""
    cols = {k: [] for k in ("source_medium", "source_matchedid", "target_medium", "target_matchedid", "relation")}
    with open(os.path.join(datadir, "media_relations.csv"), newline="") as f:
        for row in csv.DictReader(f):
            for k in cols:
                cols[k].append(row[k])
    out = {k: np.asarray([int(x) for x in v], np.int64) for k, v in cols.items() if k != "relation"}
    out["relation"] = list(cols["relation"])
    return out


def num_items(media):
    """media_relations.jl:11-15: the largest matchedid of a medium's columns + 1"""
    return int(np.max(media["matchedid"])) + 1


def get_media_details(media_by_medium):
    """media_relations.jl:17-27: {(medium, matchedid): {"mediatype": ...}} over the columns of both media (a later row wins)"""
    d = {}
    for cols in media_by_medium.values():
        for m, i, t in zip(cols["medium"], cols["matchedid"], cols["mediatype"]):
            d[(int(m), int(i))] = {"mediatype": t}
    return d


def get_media_relations(relations, details):
    """media_relations.jl:29-59: a copy of the relation columns whose "unknown" rows are reclassified: cross-medium -> "adaptation";
    same medium with one side in the manga types and the other in the novel types -> "adaptation"; otherwise left "unknown"."""
    rel = list(relations["relation"])
    for k, r in enumerate(rel):
        if r != "unknown":
            continue
        m1, id1 = int(relations["source_medium"][k]), int(relations["source_matchedid"][k])
        m2, id2 = int(relations["target_medium"][k]), int(relations["target_matchedid"][k])
        if m1 != m2:
            rel[k] = "adaptation"
            continue
        for key in ((m1, id1), (m2, id2)):
            if key not in details:
                raise ValueError(f"get_media_relations: no media details for (medium, matchedid) = {key}")
        d1, d2 = details[(m1, id1)]["mediatype"], details[(m2, id2)]["mediatype"]
        if (d1 in MANGA_TYPES and d2 in NOVEL_TYPES) or (d1 in NOVEL_TYPES and d2 in MANGA_TYPES):
            rel[k] = "adaptation"
    out = {k: np.array(v) for k, v in relations.items() if k != "relation"}
    out["relation"] = rel
    return out


# ---------------------------------------------------------------- binary sparse matrices
def _csc_from_pairs(rows, cols, shape):
    """binary CSC of the (row, col) pairs (duplicates collapse), rows ascending within each column"""
    rows = np.asarray(rows, np.int64).reshape(-1)
    cols = np.asarray(cols, np.int64).reshape(-1)
    if rows.size and (rows.min() < 0 or rows.max() >= shape[0] or cols.min() < 0 or cols.max() >= shape[1]):
        raise ValueError(f"relation ids outside the matrix shape {shape}")
    key = np.unique(cols * shape[0] + rows)
    c, r = np.divmod(key, shape[0])
    indptr = np.zeros(shape[1] + 1, np.int64)
    np.cumsum(np.bincount(c, minlength=shape[1]), out=indptr[1:])
    return indptr, r.astype(np.int32), np.ones(r.size, np.float32), (int(shape[0]), int(shape[1]))


def csc_pairs(a):
    """(rows, cols) int64 of the stored non-zeros of a CSC tuple, column-major order (SparseArrays.findnz)"""
    indptr, indices, data, shape = a
    cols = np.repeat(np.arange(shape[1], dtype=np.int64), np.diff(np.asarray(indptr, np.int64)))
    keep = np.asarray(data) != 0
    return np.asarray(indices, np.int64)[keep], cols[keep]


def csc_dense(a, dtype=np.float32):
    """dense array of a CSC tuple"""
    indptr, indices, data, shape = a
    out = np.zeros(shape, dtype)
    rows, cols = np.asarray(indices, np.int64), np.repeat(np.arange(shape[1]), np.diff(np.asarray(indptr, np.int64)))
    np.add.at(out, (rows, cols), np.asarray(data, dtype))
    return out


def get_relations(relations, source_medium, target_medium, kinds, shape):
    """media_relations.jl:61-80: the binary V_source x V_target matrix of the (reclassified) relations of the given kinds"""
    kinds = set(kinds)
    sel = np.asarray([r in kinds for r in relations["relation"]], bool).reshape(-1)
    sel &= (np.asarray(relations["source_medium"]) == source_medium) & (np.asarray(relations["target_medium"]) == target_medium)
    return _csc_from_pairs(np.asarray(relations["source_matchedid"])[sel], np.asarray(relations["target_matchedid"])[sel], shape)


def _sccs(n, rows, cols):
    """strongly connected components of the graph row -> col (iterative Tarjan): (component id per node, components in reverse
    topological order: every edge leaves a component for one listed earlier)"""
    order = np.argsort(rows, kind="stable")
    succ_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=succ_ptr[1:])
    succ = cols[order].tolist()
    succ_ptr = succ_ptr.tolist()
    index, low, comp = [-1] * n, [0] * n, [-1] * n
    on_stack, stack, comps = [False] * n, [], []
    counter = 0
    for root in sorted(set(rows.tolist())):
        if index[root] >= 0:
            continue
        work = [(root, succ_ptr[root])]
        index[root] = low[root] = counter; counter += 1
        stack.append(root); on_stack[root] = True
        while work:
            v, k = work[-1]
            if k < succ_ptr[v + 1]:
                work[-1] = (v, k + 1)
                w = succ[k]
                if index[w] < 0:
                    index[w] = low[w] = counter; counter += 1
                    stack.append(w); on_stack[w] = True
                    work.append((w, succ_ptr[w]))
                elif on_stack[w]:
                    low[v] = min(low[v], index[w])
                continue
            work.pop()
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])
            if low[v] == index[v]:
                members = []
                while True:
                    w = stack.pop(); on_stack[w] = False
                    comp[w] = len(comps); members.append(w)
                    if w == v:
                        break
                comps.append(members)
    return comp, comps


def transitive_closure(S):
    """media_relations.jl:82-93: the fixpoint of closure | (closure * closure > 0), i.e. (i, j) is set when a path of >= 1 edges leads
    from i to j (so (i, i) when i lies on a cycle).  Computed from the strongly connected components and the reachability of their
    condensation, not by dense squaring."""
    rows, cols = csc_pairs(S)
    shape = S[3]
    if shape[0] != shape[1]:
        raise ValueError("transitive_closure: the matrix must be square")
    n = shape[0]
    if rows.size == 0:
        return _csc_from_pairs(rows, cols, shape)
    comp, comps = _sccs(n, rows, cols)
    comp_a = np.asarray(comp, np.int64)
    cr, cc = comp_a[rows], comp_a[cols]
    cyclic = np.zeros(len(comps), bool)
    cyclic[cr[cr == cc]] = True                                 # an internal edge: every member reaches every member
    out_edges = {}
    for a, b in set(zip(cr[cr != cc].tolist(), cc[cr != cc].tolist())):
        out_edges.setdefault(a, []).append(b)
    members = [np.asarray(sorted(m), np.int64) for m in comps]
    reach = [None] * len(comps)                                 # nodes reachable by >= 1 edge from the component's members
    for c in range(len(comps)):                                 # successors come first (reverse topological order)
        parts = [members[c]] if cyclic[c] else []
        for b in out_edges.get(c, ()):
            parts.append(members[b])
            parts.append(reach[b])
        reach[c] = np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.int64)
    R, Cc = [], []
    for c in range(len(comps)):
        if reach[c].size:
            R.append(np.repeat(members[c], reach[c].size))
            Cc.append(np.tile(reach[c], members[c].size))
    if not R:
        return _csc_from_pairs(np.zeros(0, np.int64), np.zeros(0, np.int64), shape)
    return _csc_from_pairs(np.concatenate(R), np.concatenate(Cc), shape)


def get_matrix(relations, medium, kinds, V, symmetric=False, transitive=False):
    """media_relations.jl:95-108: the binary V x V relation matrix of `medium`; symmetric: max(S, S'); transitive: its closure; the
    diagonal cleared and stored zeros dropped"""
    S = get_relations(relations, medium, medium, kinds, (V, V))
    if symmetric:
        r, c = csc_pairs(S)
        S = _csc_from_pairs(np.concatenate([r, c]), np.concatenate([c, r]), (V, V))
    if transitive:
        S = transitive_closure(S)
    r, c = csc_pairs(S)
    off = r != c
    return _csc_from_pairs(r[off], c[off], (V, V))


# ---------------------------------------------------------------- the dependency rule
def popularity(media, V):
    """per item the sum over sources of the per-source maximum count (is_more_popular's get_popularity, media_relations.jl:117-130);
    NaN for an item without a row (Julia's sum over an empty collection throws: `is_more_popular` raises for it)"""
    best = {}
    for i, s, c in zip(media["matchedid"].tolist(), media["source"], media["count"].tolist()):
        k = (i, s)
        best[k] = max(best.get(k, 0), c)
    pop = np.full(V, np.nan)
    for (i, _), c in best.items():
        if 0 <= i < V:
            pop[i] = c if np.isnan(pop[i]) else pop[i] + c
    return pop


def is_more_popular(media, cutoff, a1, a2, pop=None):
    """media_relations.jl:110-131: popularity(a1) > (popularity(a1) + popularity(a2)) * cutoff"""
    pop = popularity(media, num_items(media)) if pop is None else pop
    p1, p2 = pop[a1], pop[a2]
    if np.isnan(p1) or np.isnan(p2):
        raise ValueError(f"is_more_popular: no rows for item {a1 if np.isnan(p1) else a2}")
    return bool(p1 > (p1 + p2) * cutoff)


def startdates(media, V):
    """the startdate of each item's first row (None: no row, or an empty date)"""
    out = [None] * V
    seen = set()
    for i, d in zip(media["matchedid"].tolist(), media["startdate"]):
        if i not in seen and 0 <= i < V:
            seen.add(i)
            out[i] = d
    return out


def is_released_after(media, a1, a2, dates=None):
    """media_relations.jl:133-158: the dates split on "-" and compared field by field as strings ("2001-10" < "2001-9"); a missing
    date on either side is "not released after", and so are equal leading fields"""
    dates = startdates(media, num_items(media)) if dates is None else dates
    s1, s2 = (dates[a] if 0 <= a < len(dates) else None for a in (a1, a2))
    if s1 is None or s2 is None:
        return False
    f1, f2 = s1.split("-"), s2.split("-")
    for x, y in zip(f1, f2):
        if x > y:
            return True
        if x < y:
            return False
    return False


def watched_before(watch_order, cutoff, a1, a2):
    """media_relations.jl:199-202 over arrays of pairs: W[a1, a2] > cutoff * (W[a1, a2] + W[a2, a1]), read through `watch_order.gather`"""
    a1 = np.asarray(a1, np.int32).reshape(-1)
    a2 = np.asarray(a2, np.int32).reshape(-1)
    if a1.size == 0:
        return np.zeros(0, bool)
    w12 = np.asarray(watch_order.gather(a1, a2), np.float64)
    w21 = np.asarray(watch_order.gather(a2, a1), np.float64)
    return w12 > cutoff * (w12 + w21)


def is_watched_before(watch_order, cutoff, a1, a2):
    """media_relations.jl:199-202 for one pair"""
    return bool(watched_before(watch_order, cutoff, [a1], [a2])[0])


def remove_transitive_edges(rows, cols, shape):
    """media_relations.jl:240-248, sequentially: for each edge (i, j) of the matrix as it stood before the loop, in column-major order,
    clear it when some k has M[i, k] and M[k, j] set in the CURRENT matrix (an edge cleared earlier no longer witnesses a later one)"""
    out_of, into = {}, {}
    for i, j in zip(rows.tolist(), cols.tolist()):
        out_of.setdefault(i, set()).add(j)
        into.setdefault(j, set()).add(i)
    for i, j in zip(rows.tolist(), cols.tolist()):
        if j in out_of[i] and not out_of[i].isdisjoint(into[j]):
            out_of[i].discard(j)
            into[j].discard(i)
    r = [i for i in out_of for _ in out_of[i]]
    c = [j for i in out_of for j in out_of[i]]
    return _csc_from_pairs(np.asarray(r, np.int64), np.asarray(c, np.int64), shape)


def save_dependencies(relations, media, medium, V, watch_order):
    """media_relations.jl:204-251: M[i, j] = 1 if j should be watched before i.  R = sum of the transitive sequel / prequel /
    parent_story / side_story matrices, R + R'; an edge (i, j) of R is kept when j is more popular than i (cutoff 0.5), was watched
    before i (cutoff 0.5, `watch_order.gather`) and is not released after i; then the transitive edges are removed."""
    mats = [get_matrix(relations, medium, [x], V, transitive=True) for x in DEPENDENCY_RELATIONS]
    pr = [csc_pairs(m) for m in mats]
    r = np.concatenate([p[0] for p in pr] + [p[1] for p in pr])
    c = np.concatenate([p[1] for p in pr] + [p[0] for p in pr])
    i, j = csc_pairs(_csc_from_pairs(r, c, (V, V)))              # the pattern of R + R', column-major
    if i.size == 0:
        return _csc_from_pairs(i, j, (V, V))
    pop = popularity(media, V)
    bad = np.isnan(pop[i]) | np.isnan(pop[j])
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError(f"is_more_popular: no rows for item {int(j[k]) if np.isnan(pop[j[k]]) else int(i[k])}")
    keep = pop[j] > (pop[j] + pop[i]) * 0.5
    keep[keep] = watched_before(watch_order, 0.5, j[keep], i[keep])
    dates = startdates(media, V)
    for k in np.flatnonzero(keep):
        keep[k] = not is_released_after(media, int(j[k]), int(i[k]), dates)
    return remove_transitive_edges(i[keep], j[keep], (V, V))


def save_related(relations, medium, V):
    """media_relations.jl:253-272: i and j are in the same franchise (symmetric, transitive)"""
    return get_matrix(relations, medium, RELATED_RELATIONS, V, symmetric=True, transitive=True)


def save_recaps(relations, medium, V):
    """media_relations.jl:274-285: i and j are the same story (symmetric)"""
    return get_matrix(relations, medium, RECAP_RELATIONS, V, symmetric=True)


def save_adaptations(relations, medium, V, V_other):
    """media_relations.jl:287-291: i (of `medium`) is an adaptation of j (of the other medium): V x V_other"""
    return get_relations(relations, medium, 1 - medium, ADAPTATION_RELATIONS, (V, V_other))


def _read_inputs(datadir):
    media = {m: read_media(datadir, m) for m in MEDIA}
    relations = get_media_relations(read_media_relations(datadir), get_media_details(media))
    return media, relations


def _save_csc(d, key, a):
    indptr, indices, data, shape = a
    d[f"{key}.indptr"], d[f"{key}.indices"], d[f"{key}.data"] = indptr, indices, data
    d[f"{key}.shape"] = np.asarray(shape, np.int64)


def save_relations(datadir, m, watch_order, outdir=None):
    """media_relations.jl:293-310: writes media_relations.{m}.npz ({m}.dependencies, .related, .recaps, .adaptations as CSC parts
    "{key}.indptr / .indices / .data / .shape") to `outdir` (default `datadir`); `watch_order` is read through its `gather` (a
    `WatchOrder` handle or the `WatchCounts` of `get_watch_order`).  Returns the path."""
    media, relations = _read_inputs(datadir)
    V, Vo = num_items(media[m]), num_items(media[1 - m])
    d = {}
    _save_csc(d, f"{m}.dependencies", save_dependencies(relations, media[m], m, V, watch_order))
    _save_csc(d, f"{m}.related", save_related(relations, m, V))
    _save_csc(d, f"{m}.recaps", save_recaps(relations, m, V))
    _save_csc(d, f"{m}.adaptations", save_adaptations(relations, m, V, Vo))
    path = os.path.join(outdir or datadir, f"media_relations.{m}.npz")
    np.savez(path, **d)
    return path


def load_relations(outdir, media=(0, 1)):
    """the media_relations.{m}.npz files of `media` as one dict {"{m}.dependencies": (indptr, indices, data, shape), ...}: what
    `serve.load_retrieval_tables` and `serve.load_ranking_tables` take (a medium whose file is absent is left out)"""
    out = {}
    for m in media:
        path = os.path.join(outdir, f"media_relations.{m}.npz")
        if not os.path.exists(path):
            continue
        with np.load(path) as z:
            for kind in ("dependencies", "related", "recaps", "adaptations"):
                k = f"{m}.{kind}"
                out[k] = (z[f"{k}.indptr"], z[f"{k}.indices"], z[f"{k}.data"], tuple(int(x) for x in z[f"{k}.shape"]))
    return out


# ---------------------------------------------------------------- watch order
def project_earliest(user, medium):
    """media_relations.jl:156-172, literal: the matchedids of `medium` in list order, each at its first WATCHED occurrence (status 0
    or >= 6); an unwatched occurrence does not hide a later watched one"""
    seen, items = set(), []
    for x in user["items"]:
        if x["medium"] != medium or x["matchedid"] in seen:
            continue
        if not (x["status"] == 0 or x["status"] >= WATCHING_STATUS):
            continue
        seen.add(x["matchedid"])
        items.append(x["matchedid"])
    return items


def project_earliest_csr(users, medium):
    """`project_earliest` of every user at once: (offsets int64 [n + 1], items int32), the arguments of rsys_watch_order_add"""
    lens = np.asarray([len(u["items"]) for u in users], np.int64)
    n = int(lens.sum())
    it = [x for u in users for x in u["items"]]
    med = np.fromiter((x["medium"] for x in it), np.int64, count=n)
    mid = np.fromiter((x["matchedid"] for x in it), np.int64, count=n)
    st = np.fromiter((x["status"] for x in it), np.int64, count=n)
    uid = np.repeat(np.arange(len(users), dtype=np.int64), lens)
    sel = np.flatnonzero((med == medium) & ((st == 0) | (st >= WATCHING_STATUS)))
    out_off = np.zeros(len(users) + 1, np.int64)
    if sel.size == 0:
        return out_off, np.zeros(0, np.int32)
    key = uid[sel] * (int(mid[sel].max()) + 1) + mid[sel]
    _, first = np.unique(key, return_index=True)
    keep = sel[np.sort(first)]                                  # first watched occurrence per (user, id), list order kept
    np.cumsum(np.bincount(uid[keep], minlength=len(users)), out=out_off[1:])
    return out_off, mid[keep].astype(np.int32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class WatchOrder:
    """The rsys_watch_order_* handle: the rows [row0, row1) of the V x V watch-order matrix on the device (media_relations.jl:174-197).
    `add` takes projected histories as (offsets, items) or a list of per-user id lists."""

    def __init__(self, V, row0=0, row1=None, device=0):
        self.V, self.row0 = int(V), int(row0)
        self.row1 = self.V if row1 is None else int(row1)
        h = C.c_void_p()
        check(lib().rsys_watch_order_create(self.V, self.row0, self.row1, device, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().rsys_watch_order_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, histories):
        if isinstance(histories, tuple):
            off, items = histories
        else:
            off = np.zeros(len(histories) + 1, np.int64)
            np.cumsum([len(h) for h in histories], out=off[1:])
            items = np.concatenate([np.asarray(h, np.int32).reshape(-1) for h in histories]) if histories else np.zeros(0, np.int32)
        off = np.ascontiguousarray(off, np.int64)
        items = np.ascontiguousarray(items, np.int32)
        if off.size == 0:
            return
        check(lib().rsys_watch_order_add(self.h, off.size - 1, _ptr(off), _ptr(items)))

    def users(self):
        n = C.c_int64()
        check(lib().rsys_watch_order_users(self.h, C.byref(n)))
        return n.value

    def rows(self, row0=None, n_rows=None):
        row0 = self.row0 if row0 is None else int(row0)
        n_rows = self.row1 - row0 if n_rows is None else int(n_rows)
        out = np.empty((max(n_rows, 0), self.V), np.int32)
        check(lib().rsys_watch_order_rows_get(self.h, row0, n_rows, _ptr(out)))
        return out

    def gather(self, a, b):
        a = np.ascontiguousarray(a, np.int32).reshape(-1)
        b = np.ascontiguousarray(b, np.int32).reshape(-1)
        if a.size != b.size:
            raise ValueError("gather: a and b must have the same length")
        out = np.empty(a.size, np.int32)
        check(lib().rsys_watch_order_gather(self.h, a.size, _ptr(a), _ptr(b), _ptr(out)))
        return out

    def csr(self):
        """(indptr int64, indices int32, values int32) of the band, rows band-local"""
        nnz = C.c_int64()
        check(lib().rsys_watch_order_csr(self.h, None, None, None, 0, C.byref(nnz)))
        indptr = np.empty(self.row1 - self.row0 + 1, np.int64)
        indices = np.empty(max(nnz.value, 1), np.int32)
        values = np.empty(max(nnz.value, 1), np.int32)
        check(lib().rsys_watch_order_csr(self.h, _ptr(indptr), _ptr(indices), _ptr(values), indices.size, C.byref(nnz)))
        return indptr, indices[:nnz.value], values[:nnz.value]

    def clear(self):
        check(lib().rsys_watch_order_clear(self.h))


class WatchCounts:
    """The watch-order matrix on the host as CSR (`indptr`, `indices`, `data` int32, `shape`), with the `gather` the dependency rule
    and `pair_scores` read through"""

    def __init__(self, indptr, indices, data, shape):
        self.indptr = np.asarray(indptr, np.int64)
        self.indices = np.asarray(indices, np.int32)
        self.data = np.asarray(data, np.int32)
        self.shape = (int(shape[0]), int(shape[1]))

    def gather(self, a, b):
        a = np.asarray(a, np.int64).reshape(-1)
        b = np.asarray(b, np.int64).reshape(-1)
        out = np.zeros(a.size, np.int32)
        key = np.repeat(np.arange(self.shape[0], dtype=np.int64), np.diff(self.indptr)) * self.shape[1] + self.indices
        q = a * self.shape[1] + b
        pos = np.searchsorted(key, q)
        hit = pos < key.size
        hit[hit] = key[pos[hit]] == q[hit]
        out[hit] = self.data[pos[hit]]
        return out

    def toarray(self):
        out = np.zeros(self.shape, np.int32)
        out[np.repeat(np.arange(self.shape[0]), np.diff(self.indptr)), self.indices] = self.data
        return out


def _user_parts(datadir):
    """users/training/*/ in sorted order, each as its sorted list of msgpack files"""
    return [sorted(glob.glob(os.path.join(d, "*.msgpack"))) for d in sorted(glob.glob(os.path.join(datadir, "users", "training", "*", "")))]


def _load_users(files):
    import msgpack
    out = []
    for fn in files:
        with open(fn, "rb") as f:
            out.append(msgpack.unpackb(f.read(), raw=False, strict_map_key=False))
    return out


def get_watch_order(users_or_csr, V, medium=None, max_band_bytes=None, device=0):
    """media_relations.jl:174-197 on the device: (WatchCounts of W, num_users).  `users_or_csr`: projected histories as (offsets, items),
    a list of user dicts (projected here onto `medium`), or a data directory whose users/training/*/*.msgpack parts are streamed one
    part at a time.  When the dense V x V int32 matrix would exceed `max_band_bytes`, W is built in row bands, the histories fed again
    for each band."""
    V = int(V)
    ld = (V + 3) // 4 * 4
    band = V if max_band_bytes is None else max(1, min(V, int(max_band_bytes) // (ld * 4)))

    def feeds():
        if isinstance(users_or_csr, (str, os.PathLike)):
            if medium is None:
                raise ValueError("get_watch_order: a data directory needs the medium")
            for files in _user_parts(users_or_csr):
                yield project_earliest_csr(_load_users(files), medium)
        elif isinstance(users_or_csr, tuple):
            yield users_or_csr
        else:
            if medium is None:
                raise ValueError("get_watch_order: user dicts need the medium")
            yield project_earliest_csr(users_or_csr, medium)

    indptr, indices, data, num_users = [np.zeros(1, np.int64)], [], [], 0
    for r0 in range(0, V, band):
        r1 = min(V, r0 + band)
        w = WatchOrder(V, r0, r1, device)
        try:
            for f in feeds():
                w.add(f)
            p, i, d = w.csr()
            num_users = w.users()
        finally:
            w.close()
        indptr.append(p[1:] + indptr[-1][-1])
        indices.append(i)
        data.append(d)
    cat = (lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, t))
    return WatchCounts(np.concatenate(indptr), cat(indices, np.int32), cat(data, np.int32), (V, V)), num_users


def save_watch_order(datadir, m, outdir=None, max_band_bytes=None, device=0):
    """media_relations.jl:312-327: writes watches.{m}.npz ("{m}.watches" as CSR parts .indptr / .indices / .data / .shape, "{m}.users")
    to `outdir` (default `datadir`).  Returns (path, WatchCounts, num_users)."""
    V = num_items(read_media(datadir, m))
    W, users = get_watch_order(datadir, V, medium=m, max_band_bytes=max_band_bytes, device=device)
    path = os.path.join(outdir or datadir, f"watches.{m}.npz")
    np.savez(path, **{f"{m}.watches.indptr": W.indptr, f"{m}.watches.indices": W.indices, f"{m}.watches.data": W.data,
                      f"{m}.watches.shape": np.asarray(W.shape, np.int64), f"{m}.users": np.int64(users)})
    return path, W, users


def load_watch_order(outdir, m):
    """watches.{m}.npz -> (WatchCounts, num_users)"""
    with np.load(os.path.join(outdir, f"watches.{m}.npz")) as z:
        k = f"{m}.watches"
        return WatchCounts(z[f"{k}.indptr"], z[f"{k}.indices"], z[f"{k}.data"], tuple(z[f"{k}.shape"])), int(z[f"{m}.users"])


# ---------------------------------------------------------------- item_similarity/pairwise_dataset.jl
def smoothed_wilson_score(k, n, w):
    """pairwise_dataset.jl:80-86, vectorised: k = min(n, k); n += round_half_even(max(w - 2n, 0) * 0.05); the lower end of the Wald
    interval of k / n at level 0.95, max(0, p - z sqrt(p (1 - p) / n)), then at least eps(Float32).  n == 0 after smoothing gives
    p = 0 / 0: the result is NaN, as in the formula (Julia's max propagates NaN).  Restated from the source of HypothesisTests'
    `confint(BinomialTest(k, n); method = :wald)`; Julia is not run to pin it."""
    n = np.asarray(n, np.float64)
    k = np.minimum(n, np.asarray(k, np.float64))
    n = n + np.rint(np.maximum(np.asarray(w, np.float64) - 2 * n, 0) * 0.05)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = k / n
        lower = np.maximum(p - WILSON_Z * np.sqrt(p * (1 - p) / n), 0.0)
    return np.maximum(lower, EPS_F32)


def pair_scores(watch_order, source_ids, target_ids, count, popularity_sum):
    """the last step of aggragate_by_matchedid (pairwise_dataset.jl:126-135): watches = (W + W')[s, t], gathered through
    `watch_order.gather`, then score = smoothed_wilson_score(count, watches, popularity_sum).  Returns (score float64, watches int64)."""
    s = np.asarray(source_ids, np.int32).reshape(-1)
    t = np.asarray(target_ids, np.int32).reshape(-1)
    watches = np.asarray(watch_order.gather(s, t), np.int64) + np.asarray(watch_order.gather(t, s), np.int64)
    return smoothed_wilson_score(count, watches, popularity_sum), watches
