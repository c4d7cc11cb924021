"""CPU: the float64 restatements of the sharded-table kernels (tests/_shard_np.py) checked against each other and against exact
enumeration, so that the GPU parity tests (tests/test_gpu_shard_ops.py) compare the kernels with something that is itself pinned."""
import os

import numpy as np
import pytest

import _shard_np as sn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shard_philox.npz")


def _rows(rng, n, V):
    X = rng.standard_normal((n, V)) * 3.0
    tgt = rng.integers(0, V, n)
    lw = rng.uniform(0.2, 2.0, n); lw[1::4] = 0.0
    coef = 0.3 * lw / 2.5
    return X, tgt, lw, coef


@pytest.mark.parametrize("split", [(23,), (7, 8, 8), (0, 22, 1), (11, 0, 12), (0, 0, 23), (1,) * 23])
def test_w_range_ce_is_the_one_range_ce(split):
    rng = np.random.default_rng(sum(split) + len(split))
    n, V = 9, 23
    X, tgt, lw, coef = _rows(rng, n, V)
    X[2] += 80.0; X[3] -= 1e4; X[4, tgt[4]] += 40.0
    tgt[0] = 0; tgt[5] = V - 1
    term, dl, lse = sn.ce_full(X, tgt, lw, coef)
    col0 = np.concatenate([[0], np.cumsum(split)])
    pre = [0, 4, 4, 9] if len(split) == 3 else np.linspace(0, n, len(split) + 1).astype(int)
    r = sn.vp_ce([X[:, col0[q]:col0[q + 1]] for q in range(len(split))], col0[:-1], tgt, lw, coef, pre)
    assert np.allclose(r["lse"], lse, rtol=1e-14, atol=0)
    assert np.allclose(r["term"], term, rtol=1e-12, atol=1e-12 * np.abs(lse).max())
    assert np.isclose(r["loss"].sum(), term.sum(), rtol=1e-12)
    assert np.allclose(np.concatenate(r["dl"], 1), dl, rtol=1e-11, atol=1e-300)
    for q, v in enumerate(split):
        if v == 0:   # an empty range: the neutral elements
            assert np.all(r["lmax"][q] == float(sn.NEG)) and np.all(r["sums"][q] == 0) and np.all(r["tl"][q] == 0)
    assert np.all((r["tl"] != 0).sum(0) <= 1)   # one owner per target


def _ss_ranks(rng, X, tgt, split, n_ss, T_extra=()):
    """class lists of a full logit matrix X over column ranges `split` with n_ss[q] samples each (drawn uniformly per stratum)"""
    col0 = np.concatenate([[0], np.cumsum(split)])
    ranks = []
    for q, (length, n_s) in enumerate(zip(split, n_ss)):
        if n_s == 0:
            ranks.append(dict(X=np.zeros((len(X), 0)), cols=np.zeros(0, int), n_s=0, len=length, col0=col0[q], tgt=tgt)); continue
        lo = sn.stratum_lo(np.arange(n_s + 1), length, n_s)
        cols = np.array([rng.integers(lo[j], lo[j + 1]) for j in range(n_s)])
        T = np.zeros(0, int)
        if n_s < length:
            loc = np.concatenate([tgt, np.asarray(T_extra, int)]) - col0[q]
            T = np.unique(loc[(loc >= 0) & (loc < length)])
            cols = np.where(np.isin(cols, T), -1, cols)
        cl = np.concatenate([cols, T])
        ranks.append(dict(X=X[:, col0[q] + np.maximum(cl, 0)], cols=cl, n_s=n_s, len=length, col0=col0[q], tgt=tgt))
    return ranks


@pytest.mark.parametrize("split", [(23,), (7, 8, 8), (0, 22, 1)])
def test_sampled_estimator_with_every_class_sampled_is_the_full_softmax(split):
    rng = np.random.default_rng(len(split))
    n, V = 9, 23
    X, tgt, lw, coef = _rows(rng, n, V)
    term, dl, lse = sn.ce_full(X, tgt, lw, coef)
    ranks = _ss_ranks(rng, X, tgt, split, split)
    tl = X[np.arange(n), tgt]
    r = sn.ss_chain(ranks, tl, lw, coef, [0, n] + [n] * (len(split) - 1))
    assert np.allclose(r["lse"], lse, rtol=1e-14)
    assert np.allclose(r["term"], term, rtol=1e-12, atol=1e-13)
    assert np.allclose(r["dt"], dl[np.arange(n), tgt], rtol=1e-11, atol=1e-15)
    full = np.concatenate(r["dl"], 1)
    ref = dl.copy(); ref[np.arange(n), tgt] = 0.0      # the class list's gradient is zero at the row's own target: dt carries it
    assert np.allclose(full, ref, rtol=1e-11, atol=1e-300)


@pytest.mark.parametrize("length,n_s", [(6, 3), (7, 3), (5, 2), (7, 1), (4, 4)])
@pytest.mark.parametrize("T", [(), (1,), (0, 3, 4)])
def test_sampled_estimator_is_unbiased_by_exact_enumeration(length, n_s, T):
    """every draw has probability prod 1 / s_j: the mean of Z-hat over all draws is Z, for strata of unequal sizes, with and without
    in-batch targets, whether or not the row's own target is among them"""
    rng = np.random.default_rng(10 * length + n_s)
    l = rng.standard_normal(length) * 2.0
    sizes = sn.stratum_sizes(length, n_s)
    assert sizes.sum() == length and sizes.min() >= 1
    T = tuple(c for c in T if c < length)
    for t in range(length):
        zs = [sn.ss_z_hat(l, t, set(T), cols, n_s) for cols in sn.ss_all_draws(length, n_s)]
        assert len(zs) == np.prod(sizes)
        assert abs(np.mean(zs) - np.exp(l).sum()) <= 1e-13 * np.exp(l).sum()
    if len(set(sizes)) > 1 and not T:   # and the single global factor len / n_s is NOT unbiased where the strata differ
        zs = [np.exp(l[0]) + sum(length / n_s * np.exp(l[c]) for c in cols if c != 0) for cols in sn.ss_all_draws(length, n_s)]
        assert abs(np.mean(zs) - np.exp(l).sum()) > 1e-6 * np.exp(l).sum()


def test_ss_chain_is_z_hat():
    """the chain form (per-rank max / sum, rebase, target joined at the max) computes log of exactly the enumerated estimator"""
    rng = np.random.default_rng(4)
    n, split, n_ss = 7, (7, 0, 10), (3, 0, 4)
    V = sum(split)
    X, tgt, lw, coef = _rows(rng, n, V)
    tgt[0] = 2; tgt[1] = 2; tgt[2] = 16
    ranks = _ss_ranks(rng, X, tgt, split, n_ss)
    ranks[0]["cols"][1] = 3; ranks[0]["X"][:, 1] = X[:, 3]; tgt[3] = 3   # row 3's target is not in T: an accidental hit at entry 1
    r = sn.ss_chain(ranks, X[np.arange(n), tgt], lw, coef, [0, 3, 3, n])
    col0 = (0, 7, 7)
    for row in range(n):
        z = np.exp(X[row, tgt[row]])
        for q, rk in enumerate(ranks):
            w = sn.ss_weights(rk["len"], rk["n_s"], len(rk["cols"]))
            for c, wc in zip(rk["cols"], w):
                if c >= 0 and c + col0[q] != tgt[row]:
                    z += wc * np.exp(X[row, c + col0[q]])
        assert abs(r["lse"][row] - np.log(z)) <= 1e-13 * abs(np.log(z)) + 1e-14
    assert not r["act"][0][3, 1] and r["dl"][0][3, 1] == 0.0


def test_philox_known_answer_and_recorded_stream():
    # Random123's known-answer vector of philox4x32-10 for an all-zero counter and key
    assert [hex(int(v)) for v in sn.philox(0, 0, 0)[0]] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    assert sn.u01(np.uint32(0xFFFFFFFF)) == np.float32(1.0) - np.float32(2.0 ** -24) and sn.u01(np.uint32(255)) == 0.0
    # columns read back from ss_sample_kernel on an MI355X, recorded once: the counter layout (ctr lo, ctr hi, stream, 0), the key halves
    # and the float32 product are the kernel's
    g = np.load(GOLDEN)
    for k in range(len(g["length"])):
        length, n_s, seed, stream = int(g["length"][k]), int(g["n_s"][k]), int(g["seed"][k]), int(g["stream"][k])
        want = g["cols"][k][:n_s]
        assert np.array_equal(sn.ss_sample(length, n_s, seed, stream), want), (length, n_s, seed, stream)


def test_ss_sample_one_class_inside_each_stratum():
    for length, n_s in [(1, 1), (5, 5), (7, 3), (10, 3), (1000, 256), (200003, 4096)]:
        cols = sn.ss_sample(length, n_s, 0x1234567, 9)
        lo = sn.stratum_lo(np.arange(n_s + 1), length, n_s)
        assert np.all(cols >= lo[:-1]) and np.all(cols < lo[1:])
        assert lo[0] == 0 and lo[-1] == length and np.all(np.diff(lo) >= 1)


def test_plan_and_compact():
    rng = np.random.default_rng(0)
    V = 50
    ids = rng.integers(0, V, 200); ids[::7] = -1
    key = np.where(ids < 0, V, ids)
    sidx = np.argsort(key, kind="stable"); skey = key[sidx]
    slot, uniq, tok2u, (U, uV) = sn.plan_unique(skey, sidx, V)
    assert np.array_equal(uniq[:U], np.unique(np.concatenate([key, [V]]))) and uniq[uV] == V
    assert np.array_equal(uniq[tok2u], key) and np.array_equal(uniq[slot], skey)
    slot, uniq, tok2u, (U, uV) = sn.plan_unique(np.sort(ids[ids >= 0]), np.arange((ids >= 0).sum()), V)
    assert uniq[-1] == V and uV == U - 1 and slot.max() == U - 2        # no masked token: the mask row still gets the last slot
    bounds = [0, 10, 10, 37, V + 1]
    off = sn.plan_offsets(uniq, bounds)
    assert off[0] == 0 and off[-1] == U and off[1] == off[2]
    for o in range(4):
        assert np.all((uniq[off[o]:off[o + 1]] >= bounds[o]) & (uniq[off[o]:off[o + 1]] < bounds[o + 1]))
    nlive, pre, src = sn.vp_compact([2, 0, 3], 4)
    assert nlive == 5 and list(pre) == [0, 2, 2, 5] and src == [(0, 0), (0, 1), (2, 0), (2, 1), (2, 2)]
