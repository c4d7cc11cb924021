"""float64 numpy restatement of the search model (Training/search/train.py:76-130): the oracle of tests/test_search_host.py and
tests/test_gpu_search.py.  Written from the formulas:
  W = E Wenc^T, logits = x W^T exp(s), log-soft-max separately over the columns of medium 0 and of medium 1, w <- w / sum w,
  loss = sum_i -logp[i, y_i] w_i / sum w                                           (the reference's order, `loss_reference`)
  P = x Wenc, z = P E_m^T exp(s), loss = sum_i w_i (logsumexp(z_i) - z_i[y_i]),
  G = w_i (softmax(z_i) - onehot(y_i)), dP = exp(s) G E_m, dWenc = x^T dP, ds = sum G * z   (the factored order, `forward_backward`)"""
import math

import numpy as np


def bf16(x):
    """round to bf16 (nearest even) and back, as float64"""
    a = np.ascontiguousarray(np.asarray(x, np.float32))
    u = a.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32).astype(np.float64)


def logsumexp(z):
    m = z.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))[:, 0]


def loss_reference(E, vocab0, Wenc, s, x, matchedids, mediums, w):
    """the loss in the reference's order: E [V0 + V1][D] (medium 0's rows first), W materialised, both media's columns soft-maxed"""
    E = np.asarray(E, np.float64); Wenc = np.asarray(Wenc, np.float64); x = np.asarray(x, np.float64)
    y = np.asarray(matchedids) + np.where(np.asarray(mediums) == 1, vocab0, 0)
    w = np.asarray(w, np.float64)
    w = w / w.sum()
    W = E @ Wenc.T
    logits = x @ W.T * math.exp(s)
    logsoft = np.hstack([logits[:, :vocab0] - logsumexp(logits[:, :vocab0])[:, None],
                         logits[:, vocab0:] - logsumexp(logits[:, vocab0:])[:, None]])
    return float((-logsoft[np.arange(len(y)), y] * w).sum() / w.sum())


def forward_backward(Em, Wenc, s, x, labels, w, bf16_mode=False, skip_round=()):
    """the factored order on one medium's rows Em [V_m][D]; returns a dict: loss, lse, z (logits), dP, dWenc, ds.  bf16_mode rounds the
    device's MFMA operands: x, Wenc, E_m, P, G and the dP that enters dWenc; skip_round names roundings to leave out ("P", "G", "dP")"""
    Em = np.asarray(Em, np.float64); Wenc = np.asarray(Wenc, np.float64); x = np.asarray(x, np.float64)
    labels = np.asarray(labels)
    w = np.asarray(w, np.float64)
    wn = w / w.sum()
    if bf16_mode:
        Em, Wenc, x = bf16(Em), bf16(Wenc), bf16(x)
    es = math.exp(s)
    P = x @ Wenc
    if bf16_mode and "P" not in skip_round:
        P = bf16(P)
    z = P @ Em.T * es
    lse = logsumexp(z)
    rows = np.arange(len(labels))
    loss = float((wn * (lse - z[rows, labels])).sum())
    G = np.exp(z - lse[:, None])
    G[rows, labels] -= 1.0
    G *= wn[:, None]
    ds = float((G * z).sum())
    Gop = bf16(G) if bf16_mode and "G" not in skip_round else G
    dP = es * (Gop @ Em)
    dPop = bf16(dP) if bf16_mode and "dP" not in skip_round else dP
    dWenc = x.T @ dPop
    return {"loss": loss, "lse": lse, "z": z, "dP": dP, "dWenc": dWenc, "ds": ds, "weight_sum": float(w.sum())}


def adamw(p, g, m, v, step, lr, decay, clip, b1=0.9, b2=0.999, eps=1e-8):
    """torch AdamW after clip_grad_norm_(clip) over the concatenated gradient, with the GradScaler's skip rule: a non-finite norm
    leaves parameters, moments and the step count alone.  decay: weight decay per tensor.  Returns ([(p, m, v)], norm, new step)."""
    norm = math.sqrt(sum(float((np.asarray(x, np.float64) ** 2).sum()) for x in g))
    if not math.isfinite(norm):
        return [(pi, mi, vi) for pi, mi, vi in zip(p, m, v)], norm, step
    step += 1
    coef = min(1.0, clip / (norm + 1e-6)) if clip > 0 else 1.0
    out = []
    for pi, gi, mi, vi, di in zip(p, g, m, v, decay):
        gi = np.asarray(gi, np.float64) * coef
        pi = pi * (1 - lr * di)
        mi = b1 * mi + (1 - b1) * gi
        vi = b2 * vi + (1 - b2) * gi * gi
        pi = pi - lr / (1 - b1 ** step) * mi / (np.sqrt(vi) / math.sqrt(1 - b2 ** step) + eps)
        out.append((pi, mi, vi))
    return out, norm, step


def epoch_loss(losses, weight_sums):
    """sum loss * (raw sum w) / sum (raw sum w) (train.py:167-178)"""
    losses = np.asarray(losses, np.float64); weight_sums = np.asarray(weight_sums, np.float64)
    return float((losses * weight_sums).sum() / weight_sums.sum())


def export(Em, Wenc):
    return np.asarray(Em, np.float64) @ np.asarray(Wenc, np.float64).T


def logp(Em, Wenc, s, x, bf16_mode=False):
    """log_softmax over the medium's items of the factored logits"""
    Em = np.asarray(Em, np.float64); Wenc = np.asarray(Wenc, np.float64); x = np.asarray(x, np.float64)
    if bf16_mode:
        Em, Wenc, x = bf16(Em), bf16(Wenc), bf16(x)
    P = x @ Wenc
    if bf16_mode:
        P = bf16(P)
    z = P @ Em.T * math.exp(s)
    return z - logsumexp(z)[:, None]


def topk(scores, k):
    """the k best columns per row by descending score, ties by ascending id (stable argsort on -score)"""
    scores = np.asarray(scores)
    ids = np.argsort(-scores, axis=1, kind="stable")[:, :k]
    return ids.astype(np.int32), np.take_along_axis(scores, ids, axis=1)
