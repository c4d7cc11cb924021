"""numpy restatement of Inference/render.jl for a state WITHOUT users (compute.jl:490-514 `/add_item`: "pick a title, see similar
titles"), the host path that rsys_retrieve_window / rsys_render_items replace.

Two forms:
* `retrieval_literal` / `render_literal`: render.jl:240-333 and :365-474 line for line in float32 -- the prior accumulated per selected
  item, `p[1] = -Inf`, no users (so no relation rule runs and `ranking` returns zeros, :354), the selected items, `sortperm(p, rev =
  true)` (stable: equal scores keep ascending id) filtered by the released set, then the page window, `reranking!` on zeros with
  partialk = the page's last index, and the page's slice.  Deviation kept from serve.page_window: the ranked slice is clamped to the list.
* `ordering_exact`: the vectorised oracle of the GPU tests on INTEGER-valued tables (`integer_tables`): the prior in int64, then
  np.lexsort((id, -p)) over the admissible items.  With entries of E in {-3..3}, crossproject in {-1, 0, 1} and dim = 8 every fp32 dot
  product is an exact integer below 2^24 in any summation order, so float32 arithmetic of any order reproduces it exactly and equality
  is the bound.  E's rows are drawn from 7 distinct vectors (vector 1 = -vector 0), so a medium's scores take at most 7 values and tie
  blocks of hundreds of items straddle every window edge.

Julia is not in the image: the forms are restated from render.jl's source.  Conventions as tests/_render_retrieval_np.py.
"""
import numpy as np

import _render_rank_np as rk

MAX_ITEMS_TO_RANK = 1024     # render.jl:448
N_VECTORS = 7


def integer_tables(rng, V, dim=8):
    """(item_similarity dict in Julia's layout, which): embeddings.{m} (dim, V_m) with columns drawn from N_VECTORS distinct integer
    vectors in {-3..3}^dim, crossproject.{m} (dim, dim) in {-1, 0, 1}; which[m][i] = the vector item i of medium m carries"""
    while True:
        base = rng.integers(-3, 4, (N_VECTORS, dim))
        base[1] = -base[0]
        if len({tuple(b) for b in base}) == N_VECTORS and base[0].any():
            break
    sim, which = {}, {}
    for m in (0, 1):
        which[m] = rng.integers(0, N_VECTORS, V[m])
        sim[f"embeddings.{m}"] = np.ascontiguousarray(base[which[m]].T, np.float32)
        sim[f"crossproject.{m}"] = rng.integers(-1, 2, (dim, dim)).astype(np.float32)
    return sim, which


def prior_int(m, sim, state, V):
    """render.jl:241-252 in int64 (integer tables only)"""
    Em = np.asarray(sim[f"embeddings.{m}"]).astype(np.int64)
    s = np.zeros(Em.shape[0], np.int64)
    for a in state["items"]:
        am = int(a["medium"])
        x = np.asarray(sim[f"embeddings.{am}"]).astype(np.int64)[:, int(a["matchedid"])]
        if am != m:
            x = np.asarray(sim[f"crossproject.{am}"]).astype(np.int64) @ x
        s += x
    return Em.T @ s


def admissible(m, state, V, released=None):
    """everything except item 0, the selected items of medium m and the unreleased items"""
    adm = np.ones(V[m], bool)
    adm[0] = False
    for a in state["items"]:
        if int(a["medium"]) == m:
            adm[int(a["matchedid"])] = False
    if released is not None:
        adm &= np.asarray(released, bool)
    return adm


def ordering_exact(m, sim, state, V, released=None):
    """(ids, scores float32) of the whole ordering of a user-less state on integer tables: descending score, ties by ascending id"""
    p = prior_int(m, sim, state, V)
    ids = np.flatnonzero(admissible(m, state, V, released))
    order = np.lexsort((ids, -p[ids]))
    ids = ids[order]
    return ids.astype(np.int32), p[ids].astype(np.float32)


def retrieval_literal(m, sim, state, V, released=None):
    """render.jl:240-333 for a state without users, float32"""
    assert not state["users"]
    p = np.zeros(V[m], np.float32)                                            # :242
    Em = np.asarray(sim[f"embeddings.{m}"], np.float32)
    for a in state["items"]:                                                  # :243-252
        am = int(a["medium"])
        if m == am:
            x = Em[:, int(a["matchedid"])]
        else:
            x = np.asarray(sim[f"embeddings.{am}"], np.float32)[:, int(a["matchedid"])]
            x = np.asarray(sim[f"crossproject.{am}"], np.float32) @ x
        p = p + Em.T @ x
    p[0] = -np.inf                                                            # :256
    for a in state["items"]:                                                  # :323-328
        if m == int(a["medium"]):
            p[int(a["matchedid"])] = -np.inf
    ids = np.argsort(-p, kind="stable")                                       # :330 (a stable sort: ties keep ascending id)
    keep = [i for i in ids if (released is None or released[i]) and p[i] > -np.inf]   # :331
    return np.asarray(keep, np.int32), p


def page_window(total, pagination):
    """render.jl:448-463: (start, stop, sidx, eidx) with sidx / eidx 1-based within the slice, or None for a page past the list"""
    mitr = MAX_ITEMS_TO_RANK - MAX_ITEMS_TO_RANK % pagination["limit"]        # :448-449
    sidx = pagination["offset"] + 1                                           # :451
    eidx = pagination["offset"] + pagination["limit"]
    if sidx > total:                                                          # :453
        return None
    if eidx > total:
        eidx = total
    page = (sidx - 1) // mitr                                                 # :460
    start, stop = page * mitr, min((page + 1) * mitr, total)                  # :461, clamped
    return start, stop, sidx - page * mitr, eidx - page * mitr


def render_literal(state, pagination, sim, related, V, released=None):
    """render.jl:437-474 for a state without users: (ids of the page, total)"""
    m = int(state["medium"])
    idxs, _ = retrieval_literal(m, sim, state, V, released)                   # :447
    total = len(idxs)
    win = page_window(total, pagination)
    if win is None:
        return np.zeros(0, np.int32), total
    start, stop, sidx, eidx = win
    idxs = idxs[start:stop]
    r = np.zeros(len(idxs), np.float32)                                       # :354, no users
    emb = np.asarray(sim[f"embeddings.{m}"], np.float32).T
    ids = rk.reranking(state, idxs, r, eidx, related[f"{m}.related"], emb)    # :470
    return np.asarray(ids[sidx - 1:eidx], np.int32), total
