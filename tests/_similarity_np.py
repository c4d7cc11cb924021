"""float64 numpy restatement of the item-similarity LambdaRank model (Training/item_similarity/pairwise_ltr.py) and of Finetune/pairwise.jl's
cross-medium map: the oracle of tests/test_similarity_host.py and tests/test_gpu_similarity.py."""
import math

import numpy as np


def bf16(x):
    """round to bf16 (nearest even) and back, as float64"""
    a = np.ascontiguousarray(np.asarray(x, np.float32))
    u = a.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32).astype(np.float64)


def encode(feat, ids, W, mask=None, p=0.1, bf16_mode=False):
    """normalize(W dropout(f[ids])) and the pre-normalisation output y; mask: keep mask of the gathered rows (1 = kept)"""
    X = np.asarray(feat, np.float64)[np.asarray(ids)]
    if mask is not None:
        X = np.where(mask, (X.astype(np.float32) * np.float32(1.0 / (1.0 - p))).astype(np.float64), 0.0)
    Wd = np.asarray(W, np.float64)
    if bf16_mode:
        X, Wd = bf16(X), bf16(Wd)
    Y = X @ Wd.T
    if bf16_mode:
        Y = bf16(Y)
    return Y, X


def normalize(Y):
    n = np.maximum(np.linalg.norm(Y, axis=-1, keepdims=True), 1e-12)
    return Y / n


def ranks(x):
    """1-based descending order, ties by slot (stable), -0.0 == +0.0"""
    x = np.asarray(x, np.float64)
    order = np.argsort(-x, axis=-1, kind="stable")
    r = np.empty_like(order)
    np.put_along_axis(r, order, np.arange(1, x.shape[-1] + 1)[None, :].repeat(x.shape[0], 0), axis=-1)
    return r


def lambdarank(x, y, w, order=None):
    """(loss, dL/dx) of pairwise_ltr.py:183-190 in fp64; order: the ranks to use (default: ranks(x))"""
    x = np.asarray(x, np.float64); y = np.asarray(y, np.float64); w = np.asarray(w, np.float64)
    order = ranks(x) if order is None else order
    D = 1.0 / np.log2(1.0 + order)
    dx = x[:, :, None] - x[:, None, :]
    c = np.abs((D[:, :, None] - D[:, None, :]) * (y[:, :, None] - y[:, None, :])) * (y[:, :, None] > y[:, None, :])
    sp = np.logaddexp(0.0, -dx)            # -logsigmoid(dx)
    Lq = (c * sp).sum(axis=(1, 2))
    W = w.sum()
    sig = 1.0 / (1.0 + np.exp(dx))          # sigmoid(-dx)
    g = -(c * sig).sum(axis=2) + (c * sig).sum(axis=1)
    return float((Lq * w).sum() / W), g * (w / W)[:, None]


def forward_backward(feat, W, ls, src, tgt, rel, w, masks=None, p=0.1, bf16_mode=False):
    """training forward + backward: (loss, x, dldx, dW, dls); masks = (source-copy mask, target mask) of the rows (or None)"""
    nq, n = tgt.shape
    sid = np.repeat(np.asarray(src), n)
    Ys, Xs = encode(feat, sid, W, None if masks is None else masks[0], p, bf16_mode)
    Yt, Xt = encode(feat, tgt.reshape(-1), W, None if masks is None else masks[1], p, bf16_mode)
    a, b = normalize(Ys), normalize(Yt)
    s = math.exp(ls)
    dot = (a * b).sum(-1)
    x = (dot * s).reshape(nq, n)
    loss, g = lambdarank(x, rel, w)
    gd = (g.reshape(-1) * s)[:, None]
    nu = np.maximum(np.linalg.norm(Ys, axis=-1, keepdims=True), 1e-12)
    nv = np.maximum(np.linalg.norm(Yt, axis=-1, keepdims=True), 1e-12)
    du = gd * (b - a * dot[:, None]) / nu
    dv = gd * (a - b * dot[:, None]) / nv
    if bf16_mode:
        du, dv = bf16(du), bf16(dv)
    dW = du.T @ Xs + dv.T @ Xt
    dls = float((g.reshape(-1) * x.reshape(-1)).sum())
    return loss, x, g, dW, dls


def forward_backward_by_id(feat, W, ls, src, tgt, rel, w, order, bf16_mode=False):
    """forward_backward without dropout at large shapes: every id is encoded once, the lists are walked one query at a time, and dW
    is formed from the per-id sums of the (rounded) dY rows; order: the ranks to use, [n_q][n]"""
    nq, n = tgt.shape
    ids, inv = np.unique(np.concatenate([np.asarray(src), tgt.reshape(-1)]), return_inverse=True)
    Yu, Xu = encode(feat, ids, W, bf16_mode=bf16_mode)
    si, ti = inv[:nq], inv[nq:].reshape(nq, n)
    nrm = np.maximum(np.linalg.norm(Yu, axis=-1, keepdims=True), 1e-12)
    Un = Yu / nrm
    s = math.exp(ls)
    w = np.asarray(w, np.float64)
    Wsum = w.sum()
    A = np.zeros_like(Yu)
    x = np.zeros((nq, n)); g = np.zeros((nq, n))
    loss = 0.0
    for q in range(nq):
        a, b = Un[si[q]][None, :], Un[ti[q]]
        dot = b @ a[0]
        x[q] = dot * s
        lq, gq = lambdarank(x[q:q + 1], rel[q:q + 1], w[q:q + 1], order[q:q + 1])
        loss += lq * w[q] / Wsum
        g[q] = gq[0] * w[q] / Wsum
        gd = (g[q] * s)[:, None]
        du = gd * (b - a * dot[:, None]) / nrm[si[q]]
        dv = gd * (a - b * dot[:, None]) / nrm[ti[q]]
        if bf16_mode:
            du, dv = bf16(du), bf16(dv)
        A[si[q]] += du.sum(0)
        np.add.at(A, ti[q], dv)
    dW = A.T @ Xu
    dls = float((g * x).sum())
    return loss, x, g, dW, dls


def scores_eval(feat, W, ls, src, tgt, bf16_mode=False):
    nq, n = tgt.shape
    Ys, _ = encode(feat, np.asarray(src), W, bf16_mode=bf16_mode)
    Yt, _ = encode(feat, tgt.reshape(-1), W, bf16_mode=bf16_mode)
    a = np.repeat(normalize(Ys), n, axis=0)
    return ((a * normalize(Yt)).sum(-1) * math.exp(ls)).reshape(nq, n)


def ndcg(x, y, w):
    """(sum w nDCG, sum w) of pairwise_ltr.py:192-208, sorts stable"""
    x = np.asarray(x, np.float64); y = np.asarray(y, np.float64); w = np.asarray(w, np.float64)
    n = x.shape[1]
    disc = np.log2(np.arange(2.0, n + 2.0))
    ry = np.take_along_axis(y, np.argsort(-x, axis=1, kind="stable"), axis=1)
    iy = -np.sort(-y, axis=1)
    nd = (ry / disc).sum(1) / (iy / disc).sum(1)
    return float((nd * w).sum()), float(np.sum(w))


def adamw(p, g, m, v, step, lr, decay, clip, b1=0.9, b2=0.999, eps=1e-8):
    """torch AdamW after clip_grad_norm_(clip) over the concatenated gradient; decay: per-element weight decay"""
    norm = math.sqrt(sum(float((x.astype(np.float64) ** 2).sum()) for x in g))
    coef = min(1.0, clip / (norm + 1e-6))
    out = []
    for pi, gi, mi, vi, di in zip(p, g, m, v, decay):
        gi = gi * coef
        pi = pi * (1 - lr * di)
        mi = b1 * mi + (1 - b1) * gi
        vi = b2 * vi + (1 - b2) * gi * gi
        pi = pi - lr / (1 - b1 ** step) * mi / (np.sqrt(vi) / math.sqrt(1 - b2 ** step) + eps)
        out.append((pi, mi, vi))
    return out, norm


def hard_negatives(scores_row, src, mask_row, split, positives, n):
    """load_hard_negatives' selection (pairwise_ltr.py:76-82) with a stable argsort"""
    w = np.asarray(scores_row, np.float64).copy()
    w[src] = -np.inf
    w[mask_row if split == "training" else ~mask_row] = -np.inf
    for v in positives:
        w[v] = -np.inf
    return np.argsort(w, kind="stable")[-n:].astype(np.int32)


def group_queries(cliptype, source, popularity, target, score, testmask, datasplit):
    """LTRDataset.load_queries restated: pandas groupby (sorted keys, rows in order) + a stable sort by score descending"""
    keys = sorted(set(zip(cliptype, source, popularity)))
    out = []
    for k in keys:
        rows = [i for i in range(len(source)) if (cliptype[i], source[i], popularity[i]) == k]
        t = [(int(target[i]), float(score[i])) for i in rows if (datasplit == "test") == bool(testmask[source[i], target[i]])]
        t = sorted(t, key=lambda z: z[1], reverse=True)
        if t:
            out.append({"sourceid": int(k[1]), "popularity": math.sqrt(k[2]), "targets": t})
    return out


def closest_orthogonal_map(A, B):
    U, _, Vt = np.linalg.svd(B @ A.T)
    return U @ Vt
