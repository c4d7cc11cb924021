"""numpy restatement of Inference/render.jl:335-435 (`ranking(state, idxs)` and `reranking!(state, idxs, r, partialk)`), the host path that
rsys_rank_request replaces.

* `reranking_given`: the greedy loop of reranking! line for line in float32 on a given score row `r`, Gram matrix, same-series pairs
  and related flags: score = ((r - mmr) - ss) - rel, Julia's `argmax` (findmax under isless: -Inf < ... < -0.0 < +0.0 < ... < Inf < NaN,
  the first index wins), r[best] = -Inf, then the three penalty updates, each operation rounded in float32, and Julia's `max` (NaN
  propagates, max(-0.0, +0.0) = +0.0).  Picks repeat once fewer finite scores than rounds remain, as in render.jl.
* `reranking`: reranking! itself, with the Gram matrix `embs' * embs` in float32 and the pairs / flags read from "{m}.related".
* `ranking_fp64`: ranking's score in float64 (the yardstick of the device's fp32 score), with render.jl's log(0) = -Inf where
  coef * exp(z - lse) underflows in float32.

Julia is not in the image: the forms are restated from render.jl's source.  Conventions as tests/_render_retrieval_np.py: ids are
0-based medium-local; "{m}.related" is a 0-based CSC tuple (indptr, indices, data, shape); positions are 0-based (render.jl's 1-based
`bestid` minus one).
"""
import numpy as np

F32 = np.float32
STATUS_DELETED, STATUS_PLANNED = 3, 5


def isless_key(x):
    """uint64 keys whose order is Julia's isless on float32 (every NaN the largest, all NaNs equal)"""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    k = np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(x), np.uint64(0xFFFFFFFF), k)


def jl_argmax(x):
    """Julia's argmax(x) (0-based): the first position of the isless-maximum"""
    return int(np.argmax(isless_key(x)))


def jl_max(x, y):
    """Julia's elementwise max.(x, y) on float32"""
    x = np.asarray(x, F32); y = np.asarray(y, F32)
    out = np.where(x > y, x, y)
    eq = x == y
    out = np.where(eq, np.where(np.signbit(x), y, x), out)
    return np.where(np.isnan(x) | np.isnan(y), F32(np.nan), out).astype(F32)


def pair_matrix(related, idxs):
    """P[i, j] = candidate i is a stored nonzero row of column idxs[j] of `related` (the same-series pairs)"""
    indptr, indices, data, _ = related
    pos = {int(x): i for i, x in enumerate(idxs)}
    P = np.zeros((len(idxs), len(idxs)), bool)
    for j, c in enumerate(idxs):
        for k in range(indptr[c], indptr[c + 1]):
            if data[k] != 0 and int(indices[k]) in pos:
                P[pos[int(indices[k])], j] = True
    return P


def related_flags(related, idxs, users, medium):
    """render.jl:395-408: every list entry of `medium` whose status is not deleted / planned, of every user, flags the candidates that
    are stored nonzero rows of its column (every entry of the list, not the last status per item)"""
    indptr, indices, data, _ = related
    pos = {int(x): i for i, x in enumerate(idxs)}
    flags = np.zeros(len(idxs), bool)
    for u in users:
        for x in u["user"]["items"]:
            if int(x["medium"]) != medium or int(x["status"]) in (STATUS_DELETED, STATUS_PLANNED):
                continue
            c = int(x["matchedid"])
            for k in range(indptr[c], indptr[c + 1]):
                if data[k] != 0 and int(indices[k]) in pos:
                    flags[pos[int(indices[k])]] = True
    return flags


def reranking_given(r, G, pairs, flags, partialk, decay, mmr_penalty, same_series_penalty, related_penalty):
    """render.jl:420-430 on given inputs; returns the picked positions (0-based) in order"""
    r = np.array(r, F32)
    n = r.size
    G = np.asarray(G, F32)
    decay, mmr_p, ss_p, rel_p = F32(decay), F32(mmr_penalty), F32(same_series_penalty), F32(related_penalty)
    mmr = np.zeros(n, F32); ss = np.zeros(n, F32); rel = np.zeros(n, F32)
    rid = np.asarray(flags, bool).astype(F32)
    picks = []
    with np.errstate(all="ignore"):
        for _ in range(min(int(partialk), n)):
            score = ((r - mmr) - ss) - rel
            best = jl_argmax(score)
            picks.append(best)
            r[best] = -np.inf
            ss = ss * decay
            hit = np.asarray(pairs)[:, best]
            ss[hit] = ss[hit] + ss_p
            rel = rel * decay
            if rid[best] != 0:
                rel = rel + rid * rel_p
            mmr = jl_max(mmr * decay, G[:, best] * mmr_p)
    return picks


def reranking(state, idxs, r, partialk, related, emb):
    """reranking! itself: `emb` the (V_m, dim) item-similarity rows (Julia's "embeddings.{m}" transposed); returns the picked ids"""
    idxs = np.asarray(idxs)
    E = np.asarray(emb, F32)[idxs].T
    G = E.T @ E
    p = state["penalties"]
    picks = reranking_given(r, G, pair_matrix(related, idxs), related_flags(related, idxs, state["users"], int(state["medium"])),
                            partialk, p["decay"], p["mmr_penalty"], p["same_series_penalty"], p["related_penalty"])
    return idxs[picks]


def ranking_fp64(F, queries, r_masked, idxs, coef=None, rating_coefs=None, rating_mean=0.0):
    """render.jl:355-361 in float64: sum over users of log(coef * softmax(F u)[idxs]) + (c0 * mean + c1 * r_masked); F (V_m, D) the
    operands the device scores with (bf16-rounded in bf16 mode), -Inf where coef * exp(z - lse) is 0 in float32"""
    F = np.asarray(F, np.float64)
    idxs = np.asarray(idxs)
    c = 1.0 if coef is None else float(coef)
    score = np.zeros(idxs.size)
    for q, rm in zip(queries, r_masked):
        z = F @ np.asarray(q, np.float64)
        zmax = z.max()
        d = z[idxs] - (zmax + np.log(np.exp(z - zmax).sum()))
        with np.errstate(divide="ignore"):
            lp = np.where(F32(c) * np.exp(d).astype(F32) == 0, -np.inf, d + np.log(c))
        rm = np.asarray(rm, np.float64)
        r = rm if rating_coefs is None else rating_coefs[0] * rating_mean + rating_coefs[1] * rm
        score = score + (lp + r)
    return score
