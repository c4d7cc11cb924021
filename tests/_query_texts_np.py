"""numpy float32 twin of the text-query terms of a request (rsys_query_texts_set), on the operations of
tests/_query_weights_np.py: every operation one float32 rounding, a weight of +0.0 or -0.0 skips its term.  A text t holds its logits
z_t over the medium's items and lse_t; its term at item i is fsub(z_t[i], lse_t).  The three chains, as the kernels run them:
    retrieval   s = prior, then s = fadd(s, fmul(w_t, term_t)) in text order, then the users' terms in query order
    user-less   the same without users (rsys_retrieve_window / rsys_render_items: prior + texts)
    ranking     s = +0.0, then the texts at the candidates in text order, then s = fadd(s, fmul(w_u, lp_u + r_u)) in user order
"""
import numpy as np

import _query_weights_np as qw

f32 = np.float32


def text_terms(z, lse, ids=None):
    """fsub(z_t[ids], lse_t) per text, rows of one length (ids None: every item)"""
    if len(lse) == 0:
        return []
    z = np.asarray(z, f32).reshape(len(lse), -1)
    return [qw.fsub(z[t] if ids is None else z[t][ids], lse[t]) for t in range(len(lse))]


def _ones(w, n):
    return [f32(1.0)] * n if w is None else list(w)


def retrieval(prior, z, lse, text_w=None, user_rows=(), user_w=None):
    """the group score row before the masks: prior, the texts, then the users' rows (z_q - lse_q, float32, one per user)"""
    s = qw.chain(prior, text_terms(z, lse), _ones(text_w, len(lse)))
    return qw.chain(s, list(user_rows), _ones(user_w, len(user_rows)))


def userless(prior, z, lse, text_w=None):
    return retrieval(prior, z, lse, text_w)


def ranking(z, lse, cand, text_w=None, user_terms=(), user_w=None):
    """the ranking score at the candidates `cand`: +0.0, the texts, then the users' terms lp_u + r_u (one float32 row per user)"""
    s = qw.chain(np.zeros(len(cand), f32), text_terms(z, lse, np.asarray(cand)), _ones(text_w, len(lse)))
    return qw.chain(s, list(user_terms), _ones(user_w, len(user_terms)))
