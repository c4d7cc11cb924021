"""numpy restatement of Inference/render.jl:240-331 (`retrieval(state)`), the host path that rsys_retrieve_request replaces.

Two forms:
* `literal`: render.jl line for line -- float32 dense vectors and float32 dense relation products in render.jl's order, masks as
  `-Inf` assignments into `p`;
* `set_mask`: the reachability form the device computes -- per user the last status of each (medium, id), the sets W_m / W_o / C_m /
  K_m, and "product != 0" read as "row i has a stored nonzero entry in a column of the set", as exact booleans.

Julia is not in the image, so neither form can be pinned by running render.jl itself; they are restated from its source, and the
tests check that the two forms agree with each other and that the device agrees with them.

Conventions: ids are 0-based medium-local (render.jl's `matchedid`; its `p[x]` with x = matchedid + 1 is `p[matchedid]` here).
A relation matrix is a 0-based CSC tuple (indptr, indices, data, shape).  `item_similarity["embeddings.{m}"]` is Julia's dim x V_m
matrix, `item_similarity["crossproject.{m}"]` the dim x dim matrix as Julia indexes it.  A state is render.jl's dict: "medium",
"items" (selected: {"medium", "matchedid"}), "users" ({"user": {"items": [{"medium", "matchedid", "status"}, ...]}, ...}).
"""
import numpy as np

# Inference/render.jl:13-23
STATUS = dict(none=0, wont_watch=1, dropped=2, deleted=3, on_hold=4, planned=5, currently_watching=6, completed=7, rewatching=8)


def dense(csc):
    """float32 dense matrix of a CSC tuple (duplicate entries add, as SparseArrays.sparse does)"""
    indptr, indices, data, shape = csc
    A = np.zeros(shape, np.float32)
    for c in range(shape[1]):
        for j in range(indptr[c], indptr[c + 1]):
            A[indices[j], c] += np.float32(data[j])
    return A


def prior_literal(m, item_similarity, state, V):
    """render.jl:241-253: p += embeddings.$m' * x for every selected item, in float32 and in list order"""
    p = np.zeros(V[m], np.float32)
    Em = np.asarray(item_similarity[f"embeddings.{m}"], np.float32)
    for a in state["items"]:
        am = int(a["medium"])
        x = np.asarray(item_similarity[f"embeddings.{am}"], np.float32)[:, int(a["matchedid"])]
        if am != m:
            x = np.asarray(item_similarity[f"crossproject.{am}"], np.float32) @ x
        p += Em.T @ x
    return p


def prior_fp64(m, item_similarity, state, V):
    """the same prior in float64 (E_m^T sum_a x_a), the yardstick for the device's fp32 prior"""
    s = None
    for a in state["items"]:
        am = int(a["medium"])
        x = np.asarray(item_similarity[f"embeddings.{am}"], np.float64)[:, int(a["matchedid"])]
        if am != m:
            x = np.asarray(item_similarity[f"crossproject.{am}"], np.float64) @ x
        s = x if s is None else s + x
    if s is None:
        return np.zeros(V[m])
    return np.asarray(item_similarity[f"embeddings.{m}"], np.float64).T @ s


def literal(m, relations, state, V, p=None, released=None):
    """render.jl:254-331 on p (float32, default zeros; the prior and the users' log-probabilities, render.jl:241-256, are the
    caller's): every -Inf assignment in render.jl's order.  Returns (p with -Inf, admissible): admissible = p > -Inf and released
    (render.jl:331's `(i - 1) in keys(info) && p[i] > -Inf`), `released` a bool mask or None (all released)."""
    n = V[m]
    p = np.zeros(n, np.float32) if p is None else np.array(p, np.float32)
    dep, rec, ada = (dense(relations[f"{m}.{k}"]) for k in ("dependencies", "recaps", "adaptations"))
    p[0] = -np.inf                                                            # render.jl:255
    for u in state["users"]:                                                  # render.jl:256-323
        statuses = {0: {}, 1: {}}
        for x in u["user"]["items"]:
            statuses[int(x["medium"])][int(x["matchedid"])] = int(x["status"])
        for x, s in statuses[m].items():                                      # watched (262-266)
            if s not in (STATUS["deleted"], STATUS["planned"]):
                p[x] = -np.inf
        watched = {y: np.zeros(V[y], np.float32) for y in (0, 1)}             # adaptations (268-282)
        for y in (0, 1):
            for x, s in statuses[y].items():
                if s not in (STATUS["deleted"], STATUS["planned"]):
                    watched[y][x] = 1
        v1 = ada @ watched[1 - m]
        v2 = dep @ watched[m]
        p[(v1 != 0) & (v2 == 0)] = -np.inf
        v = rec @ watched[m]                                                  # recaps (284-289)
        p[v != 0] = -np.inf
        v = np.zeros(n, np.float32)                                           # missing dependencies (291-303)
        for x, s in statuses[m].items():
            if s >= STATUS["completed"]:
                v[x] = 1
        v1 = dep @ v
        v2 = dep @ np.ones(n, np.float32)
        p[(v2 != 0) & (v1 == 0)] = -np.inf
        v = np.zeros(n, np.float32)                                           # sequels to currently watching (305-322)
        for x, s in statuses[m].items():
            if s in (STATUS["currently_watching"], STATUS["dropped"], STATUS["wont_watch"]):
                v[x] = 1
        v = dep @ v
        p[v != 0] = -np.inf
    for a in state["items"]:                                                  # selected (324-329)
        if int(a["medium"]) == m:
            p[int(a["matchedid"])] = -np.inf
    adm = p > -np.inf
    if released is not None:
        adm &= np.asarray(released, bool)
    return p, adm


def _reach(csc, cols, n_rows):
    """rows with a stored nonzero entry in one of `cols`"""
    indptr, indices, data, _ = csc
    r = np.zeros(n_rows, bool)
    for c in cols:
        seg = slice(indptr[c], indptr[c + 1])
        r[np.asarray(indices[seg])[np.asarray(data[seg]) != 0]] = True
    return r


def set_mask(m, relations, state, V, released=None):
    """the masked items of render.jl:254-331 in set form (what rsys_retrieve_request computes): True = masked"""
    n = V[m]
    dep, rec, ada = (relations[f"{m}.{k}"] for k in ("dependencies", "recaps", "adaptations"))
    dep_rows = np.zeros(n, bool)
    dep_rows[np.asarray(dep[1])[:int(dep[0][-1])][np.asarray(dep[2])[:int(dep[0][-1])] != 0]] = True
    masked = np.zeros(n, bool)
    masked[0] = True
    for u in state["users"]:
        last = {}
        for x in u["user"]["items"]:
            last[(int(x["medium"]), int(x["matchedid"]))] = int(x["status"])
        watched = lambda s: s not in (STATUS["deleted"], STATUS["planned"])
        Wm = [i for (y, i), s in last.items() if y == m and watched(s)]
        Wo = [i for (y, i), s in last.items() if y != m and watched(s)]
        Cm = [i for (y, i), s in last.items() if y == m and s >= STATUS["completed"]]
        Km = [i for (y, i), s in last.items() if y == m and s in (STATUS["currently_watching"], STATUS["dropped"], STATUS["wont_watch"])]
        w = np.zeros(n, bool)
        w[Wm] = True
        masked |= w
        masked |= _reach(ada, Wo, n) & ~_reach(dep, Wm, n)
        masked |= _reach(rec, Wm, n)
        masked |= dep_rows & ~_reach(dep, Cm, n)
        masked |= _reach(dep, Km, n)
    for a in state["items"]:
        if int(a["medium"]) == m:
            masked[int(a["matchedid"])] = True
    if released is not None:
        masked |= ~np.asarray(released, bool)
    return masked


# ---------------------------------------------------------------- random cases
def random_csc(rng, n_rows, n_cols, density, zero_frac=0.1, empty_rows=()):
    """a 0-based CSC tuple with positive values, some explicitly stored zeros, and the rows `empty_rows` left without entries"""
    nnz = int(rng.binomial(n_rows * n_cols, density))
    key = np.unique(rng.integers(0, n_rows * n_cols, nnz))             # distinct (column, row) pairs, column-major order
    col, row = key // n_rows, key % n_rows
    keep = np.ones(row.size, bool)
    keep[np.isin(row, np.asarray(list(empty_rows), np.int64))] = False
    col, row = col[keep], row[keep]
    data = rng.uniform(0.5, 2.0, row.size).astype(np.float32)
    data[rng.random(row.size) < zero_frac] = 0.0
    indptr = np.zeros(n_cols + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(col, minlength=n_cols))
    return (indptr, row.astype(np.int32), data, (n_rows, n_cols))


def random_relations(rng, V, density=0.02):
    rel = {}
    for m in (0, 1):
        empty = rng.choice(V[m], size=max(1, V[m] // 4), replace=False)
        rel[f"{m}.dependencies"] = random_csc(rng, V[m], V[m], density, empty_rows=empty)
        rel[f"{m}.recaps"] = random_csc(rng, V[m], V[m], density / 2)
        rel[f"{m}.adaptations"] = random_csc(rng, V[m], V[1 - m], density)
    return rel


def random_user_items(rng, V, n, hot=None):
    """n list items over both media with every status value; `hot` (optional) ids of medium 0 and 1 to repeat, so that one item
    appears several times with changing statuses"""
    items = []
    for _ in range(n):
        y = int(rng.integers(0, 2))
        if hot is not None and rng.random() < 0.3:
            i = int(rng.choice(hot[y]))
        else:
            i = int(rng.integers(0, V[y]))
        items.append(dict(medium=y, matchedid=i, status=int(rng.integers(0, 9))))
    return items


def random_state(rng, V, m, n_users, n_items, n_selected):
    hot = [rng.integers(0, V[0], 4), rng.integers(0, V[1], 4)]
    users = [dict(user=dict(items=random_user_items(rng, V, int(rng.integers(0, n_items + 1)), hot))) for _ in range(n_users)]
    sel = [dict(medium=int(rng.integers(0, 2)), matchedid=0) for _ in range(n_selected)]
    for a in sel:
        a["matchedid"] = int(rng.integers(0, V[a["medium"]]))
    return dict(medium=m, items=sel, users=users)
