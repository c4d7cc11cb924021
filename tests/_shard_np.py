"""Plain numpy (float64) restatements of what csrc/shard.hip computes, on the values the device buffers hold: the vocabulary-parallel
cross entropy over W column ranges, the stratified sampled soft-max estimator, the Philox stream behind its draws, the exchange plan and
the live-row packing.  tests/test_shard_np.py checks the restatements against each other on the CPU; tests/test_gpu_shard_ops.py
compares the kernels with them."""
import itertools

import numpy as np

NEG = np.float32(-3.0e38)   # the neutral element of the max all-reduce, as the kernels write it


# ------------------------------------------------------------------------------------------------ Philox4x32-10 (common.hpp)
def philox(seed, ctr, stream):
    """Philox(seed).gen(ctr, stream): uint32 [len(ctr)][4]; counter words (ctr lo, ctr hi, stream, 0), key (seed lo, seed hi)"""
    M = np.uint64(0xFFFFFFFF)
    ctr = np.atleast_1d(np.asarray(ctr, np.uint64))
    c0 = ctr & M; c1 = ctr >> np.uint64(32)
    c2 = np.full_like(c0, np.uint64(stream & 0xFFFFFFFF)); c3 = np.zeros_like(c0)
    a = np.uint64(seed & 0xFFFFFFFF); b = np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0; p1 = np.uint64(0xCD9E8D57) * c2       # 32 x 32 -> 64 bits: no overflow
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & M, p1 >> np.uint64(32), p1 & M
        c0, c1, c2, c3 = h1 ^ c1 ^ a, l1, h0 ^ c3 ^ b, l0
        a = (a + np.uint64(0x9E3779B9)) & M; b = (b + np.uint64(0xBB67AE85)) & M
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def u01(x):
    """float32 in [0, 1): the top 24 bits of x (exact: both factors are exact in fp32)"""
    return (np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


# ------------------------------------------------------------------------------------------------ strata and the sample
def stratum_lo(j, length, n_s):
    return np.asarray(j, np.int64) * length // n_s


def stratum_sizes(length, n_s):
    j = np.arange(n_s, dtype=np.int64)
    return stratum_lo(j + 1, length, n_s) - stratum_lo(j, length, n_s)


def ss_sample(length, n_s, seed, stream):
    """cols[j] = lo_j + min(size_j - 1, int(u01 * float(size_j))), the product in float32 as ss_sample_kernel forms it"""
    j = np.arange(n_s, dtype=np.int64)
    size = stratum_sizes(length, n_s)
    u = u01(philox(seed, j, stream)[:, 0])
    pick = (u * size.astype(np.float32)).astype(np.float32).astype(np.int64)
    return (stratum_lo(j, length, n_s) + np.minimum(size - 1, pick)).astype(np.int32)


# ------------------------------------------------------------------------------------------------ cross entropy, one range and W ranges
def ce_full(X, tgt, lw, coef):
    """rows of logits X [n][V] (float64), target column, label * weight and gradient coefficient per row: (loss terms [n], dlogits)"""
    X = np.asarray(X, np.float64)
    gm = X.max(1)
    lse = gm + np.log(np.exp(X - gm[:, None]).sum(1))
    r = np.arange(len(X))
    d = np.exp(X - lse[:, None]); d[r, tgt] -= 1.0
    return (lse - X[r, tgt]) * lw, coef[:, None] * d, lse


def vp_ce(blocks, col0s, tgt, lw, coef, pre):
    """The vocabulary-parallel form: blocks[q] = the logits [n][Vloc_q] of rank q's columns [col0s[q], col0s[q] + Vloc_q); pre [W + 1] =
    the row ranges the ranks own.  Returns per rank (lmax, sums relative to lmax, target logit or 0), the global maximum, the rebased sums,
    lse, the loss term of every row, the loss per owner rank, dlogits per block."""
    n = len(tgt)
    W = len(blocks)
    lmax = np.full((W, n), float(NEG)); sums = np.zeros((W, n)); tl = np.zeros((W, n))
    for q, (B, c0) in enumerate(zip(blocks, col0s)):
        B = np.asarray(B, np.float64)
        if B.shape[1] == 0:
            continue
        lmax[q] = B.max(1)
        sums[q] = np.exp(B - lmax[q][:, None]).sum(1)
        loc = tgt - c0
        own = (loc >= 0) & (loc < B.shape[1])
        tl[q, own] = B[np.nonzero(own)[0], loc[own]]
    gmax = lmax.max(0)
    reb = sums * np.exp(lmax - gmax)
    lse = gmax + np.log(reb.sum(0))
    term = (lse - tl.sum(0)) * lw
    loss = np.array([term[pre[q]:pre[q + 1]].sum() for q in range(W)])
    dl = []
    for B, c0 in zip(blocks, col0s):
        B = np.asarray(B, np.float64)
        d = np.exp(B - lse[:, None])
        loc = tgt - c0
        own = (loc >= 0) & (loc < B.shape[1])
        d[np.nonzero(own)[0], loc[own]] -= 1.0
        dl.append(coef[:, None] * d)
    return dict(lmax=lmax, sums=sums, tl=tl, gmax=gmax, reb=reb, lse=lse, term=term, loss=loss, dl=dl)


# ------------------------------------------------------------------------------------------------ the sampled estimator
def ss_weights(length, n_s, n_tot):
    """weight of class-list column c: the stratum's size for a sampled class, 1 for an in-batch target"""
    return np.concatenate([stratum_sizes(length, n_s).astype(np.float64) if n_s else np.zeros(0), np.ones(n_tot - n_s)])


def ss_active(cols, tgt_local):
    """[rows][n_tot]: the class-list entries that count for a row: not dropped (-1) and not the row's own target"""
    cols = np.asarray(cols)
    return (cols[None, :] >= 0) & (cols[None, :] != np.asarray(tgt_local)[:, None])


def ss_chain(ranks, tl, lw, coef, pre):
    """ranks[q] = dict(X [n][n_tot_q] logits of the class list, cols [n_tot_q] local classes (-1 dropped), n_s, len, col0); tl [n] = the
    target logit (known to all ranks); tgt in the dicts as medium-wide ids.  Z = exp(tl) + sum_q sum_c w_c exp(x_c) [active]:
    per rank (lmax, lsum) of x + log w, gmax = max(tl, lmax_q), sneg, lse, loss terms, dt, dlogits per rank."""
    n = len(tl)
    W = len(ranks)
    lmax = np.full((W, n), float(NEG)); lsum = np.zeros((W, n))
    act = []; ys = []
    for q, r in enumerate(ranks):
        X = np.asarray(r["X"], np.float64)
        w = ss_weights(r["len"], r["n_s"], X.shape[1])
        a = ss_active(r["cols"], r["tgt"] - r["col0"]) if X.shape[1] else np.zeros((n, 0), bool)
        y = X + np.log(np.maximum(w, 1.0))[None, :]
        act.append(a); ys.append(y)
        for row in range(n):
            if a[row].any():
                lmax[q, row] = y[row, a[row]].max()
                lsum[q, row] = np.exp(y[row, a[row]] - lmax[q, row]).sum()
    gmax = np.maximum(lmax.max(0), tl)
    sneg_q = np.where(lsum > 0, lsum * np.exp(lmax - gmax), 0.0)
    sneg = sneg_q.sum(0)
    lse = gmax + np.log(np.exp(tl - gmax) + sneg)
    term = (lse - tl) * lw
    loss = np.array([term[pre[q]:pre[q + 1]].sum() for q in range(W)])
    dt = coef * (np.exp(tl - lse) - 1.0)
    dl = [np.where(a, coef[:, None] * np.exp(y - lse[:, None]), 0.0) for a, y in zip(act, ys)]
    return dict(lmax=lmax, lsum=lsum, gmax=gmax, sneg_q=sneg_q, sneg=sneg, lse=lse, term=term, loss=loss, dt=dt, dl=dl, act=act)


def ss_target_grad(EwC, Floc, tgt_local, dt, length):
    """the target classes' rows: dF[t] += dt[row] EwC[row], d(row) += dt[row] Floc[t] for rows with a local target.  Returns the two
    additions and the sums of the magnitudes of dF's terms (what the bounds scale with)"""
    EwC = np.asarray(EwC, np.float64); Floc = np.asarray(Floc, np.float64)
    dF = np.zeros_like(Floc); dFmag = np.zeros_like(Floc); dE = np.zeros_like(EwC)
    cnt = np.zeros(len(Floc), np.int64)
    for row, t in enumerate(tgt_local):
        if 0 <= t < length:
            dF[t] += dt[row] * EwC[row]; dFmag[t] += np.abs(dt[row] * EwC[row]); cnt[t] += dt[row] != 0
            dE[row] = dt[row] * Floc[t]
    return dF, dFmag, dE, cnt


def ss_z_hat(l, t, T, cols, n_s):
    """the estimator of Z = sum exp(l) for one draw `cols` (one class per stratum) of a row with target t and in-batch target set T"""
    size = stratum_sizes(len(l), n_s)
    z = np.exp(l[t]) + sum(np.exp(l[c]) for c in T if c != t)
    return z + sum(size[j] * np.exp(l[c]) for j, c in enumerate(cols) if c not in T and c != t)


def ss_all_draws(length, n_s):
    lo = stratum_lo(np.arange(n_s + 1), length, n_s)
    return itertools.product(*[range(lo[j], lo[j + 1]) for j in range(n_s)])


# ------------------------------------------------------------------------------------------------ integer paths
def plan_unique(skey, sidx, V):
    """skey ascending (raw ids, masked = V), sidx the tokens in that order: slot per position, uniq, tok2u, (U, uV)"""
    skey = np.asarray(skey, np.int64)
    head = np.concatenate([[True], skey[1:] != skey[:-1]])
    slot = np.cumsum(head) - 1
    uniq = skey[head]
    tok2u = np.empty(len(skey), np.int64); tok2u[np.asarray(sidx)] = slot
    if uniq[-1] != V:
        uniq = np.concatenate([uniq, [V]])
    return slot.astype(np.int32), uniq.astype(np.int32), tok2u.astype(np.int32), (len(uniq), len(uniq) - 1)


def plan_offsets(uniq, bounds):
    """first slot whose id is >= each bound"""
    return np.searchsorted(np.asarray(uniq), np.asarray(bounds), side="left").astype(np.int32)


def vp_compact(counts, KB):
    """live counts per rank -> (nlive, pre [W + 1], source (rank, row) of every packed row)"""
    pre = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    src = [(q, i) for q, c in enumerate(counts) for i in range(c)]
    assert all(c <= KB for c in counts)
    return int(pre[-1]), pre, src
