"""numpy float32 twin of the weighted multi-query sums (rsys_query_weights_set).

Every operation is one float32 rounding -- `fmul`, `fadd`, `fsub` below -- and a weight of +0.0 or -0.0 skips its term, so the running
sum keeps its bits.  The three chains, as the kernels run them:
    selected sum   s = fadd(s, fmul(w_a, x_a))                       in list order
    retrieval      s = fadd(s, fmul(w_q, fsub(z_q[i], lse_q)))       in query order
    ranking        s = fadd(s, fmul(w_u, t_u)),  t_u = lp_u + r_u    in user order
and the weighted literal restatement of render.jl:240-333 / `ranking` built on tests/_render_retrieval_np.py.
"""
import numpy as np

import _render_retrieval_np as rr

f32 = np.float32


def _quiet(fn):
    def run(*a):
        with np.errstate(all="ignore"):
            return fn(*a)
    return run


fmul = _quiet(lambda a, b: (np.asarray(a, f32) * np.asarray(b, f32)).astype(f32))
fadd = _quiet(lambda a, b: (np.asarray(a, f32) + np.asarray(b, f32)).astype(f32))
fsub = _quiet(lambda a, b: (np.asarray(a, f32) - np.asarray(b, f32)).astype(f32))


def weighted_add(s, w, x):
    """s + w * x with the product and the sum rounded on their own; w == +-0.0 returns s itself"""
    w = f32(w)
    if w == 0:
        return np.asarray(s, f32)
    return fadd(s, fmul(w, x))


def chain(start, terms, weights):
    """start + sum over terms in order of w * term (rows of one length)"""
    s = np.array(start, f32)
    for t, w in zip(terms, weights):
        s = weighted_add(s, w, np.asarray(t, f32))
    return s


def combine(src, z, lse, members, w, q0=0):
    """one launch of the combine pass for one group: src [V] + the queries `members` (global indices, z holds rows q - q0)"""
    return chain(src, [fsub(z[q - q0], lse[q]) for q in members], [w[q] for q in members])


def score_key(s):
    """the order-preserving uint32 key of retrieve.hip: 0 for NaN / -inf, -0.0 as +0.0"""
    s = np.asarray(s, f32)
    ok = s > -np.inf                                           # (False for NaN)
    u = np.where(s == 0, f32(0), s).astype(f32).view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(ok, key, np.uint32(0)).astype(np.uint32)


def selected_sum(x_rows, w):
    """s_g over the rows x_a [n][dim] of one group in list order"""
    dim = np.asarray(x_rows).shape[1] if len(x_rows) else 0
    return chain(np.zeros(dim, f32), list(x_rows), w)


def rank_terms(z, lse, cand, rm, coef=None, rating_coefs=None, rating_mean=0.0):
    """lp_u + r_u of one user at its group's candidates, restated from rank_request.hip: d = z - lse, lp = d + log(coef) (-inf where
    coef * exp(d) is 0 in fp32), r = fma(c1, r_masked, c0 * mean) -- the device contracts this one product and sum -- or r_masked.
    exp / log are the host's: use only where the test controls them (coef None, or the underflow case)."""
    d = fsub(np.asarray(z, f32)[cand], lse)
    c = f32(1.0 if coef is None else coef)
    with np.errstate(all="ignore"):
        p = fmul(c, np.exp(d.astype(np.float64)).astype(f32))
        lp = np.where(p == 0, f32(-np.inf), fadd(d, np.log(c).astype(f32)))
    if rating_coefs is None:
        r = np.asarray(rm, f32)
    else:
        c0m = fmul(rating_coefs[0], rating_mean)
        r = (np.asarray(rm, np.float64) * np.float64(f32(rating_coefs[1])) + np.float64(c0m)).astype(f32)   # one rounding: an fma
    return fadd(lp, r)


# ---------------------------------------------------------------- the weighted literal restatement (render.jl:240-333, `ranking`)
def user_weights(state):
    return [f32(u.get("weight", 1.0)) for u in state["users"]]


def item_weights(state):
    return [f32(a.get("weight", 1.0)) for a in state["items"]]


def prior_weighted(m, item_similarity, state, V):
    """render.jl:241-253 with a weight per selected item, in the device's association: s = sum of w_a x_a in list order, then E_m' s"""
    Em = np.asarray(item_similarity[f"embeddings.{m}"], f32)
    rows = []
    for a in state["items"]:
        am = int(a["medium"])
        x = np.asarray(item_similarity[f"embeddings.{am}"], f32)[:, int(a["matchedid"])]
        if am != m:
            x = np.asarray(item_similarity[f"crossproject.{am}"], f32) @ x
        rows.append(x)
    if not rows:
        return np.zeros(V[m], f32)
    return (Em.T @ selected_sum(np.stack(rows), item_weights(state))).astype(f32)


def literal_weighted(m, relations, state, V, logp=None, prior=None, released=None):
    """render.jl:240-333 with weights: p = prior + sum over users of w_u * log p_u (`logp`: one float32 row per user), then every mask
    of `_render_retrieval_np.literal` -- which never reads a weight.  Returns (p with -Inf, admissible)."""
    p = np.zeros(V[m], f32) if prior is None else np.array(prior, f32)
    if logp is not None:
        p = chain(p, logp, user_weights(state))
    return rr.literal(m, relations, state, V, p=p, released=released)


def ranking_weighted(state, terms):
    """`ranking(state, idxs)` with weights: sum over users in order of w_u * (log p_u[idxs] + r_u), `terms` one row per user"""
    n = len(terms[0]) if len(terms) else 0
    return chain(np.zeros(n, f32), terms, user_weights(state))
