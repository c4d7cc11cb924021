"""CPU: the host side of the item-similarity model (recommendersystem_amd/similarity.py) against tests/_similarity_np.py: query grouping
and the stable target sort, the positive caps, list assembly, the -inf fill rule of the hard negatives, EarlyStopper and the CSV rows, the
cross-medium map and the layout of the item_similarity tables; and the restatement's own hand-derived gradients (what the GPU tests compare
the device with) against torch autograd in fp64, at ragged list lengths and on the clamp branch of the normalisation."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _similarity_np as sn  # noqa: E402

from recommendersystem_amd import similarity as sim  # noqa: E402


# ---- the oracle's hand-derived gradients against autograd (the formulas of csrc/similarity.hip's header, restated in torch fp64)
def _ltr_problem(nq, n, seed=0, v=400, f=24, e=16):
    """targets drawn without replacement, at least two distinct relevances per list (where n > 1), ties among the relevances"""
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((v, f))
    W = rng.standard_normal((e, f)) / np.sqrt(f)
    src = rng.integers(0, v, nq)
    tgt = np.stack([rng.permutation(v)[:n] for _ in range(nq)])
    rel = np.where(rng.random((nq, n)) < 0.4, rng.integers(1, 6, (nq, n)).astype(np.float64), 0.0)
    if n > 1:
        rel[:, 0], rel[:, 1] = 3.0, 0.0
    w = np.sqrt(rng.integers(1, 100, nq).astype(np.float64))
    return feat, W, math.log(1.0 / 0.07), src, tgt, rel, w


def _ltr_autograd(feat, W, ls, src, tgt, rel, w):
    """(loss, x, dL/dx, dW, dls): encoder f[id] @ W.T, F.normalize, dot product * exp(logit_scale), LambdaRank with the ranks a constant"""
    torch = pytest.importorskip("torch")
    nq, n = tgt.shape
    tW = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    tls = torch.tensor(ls, dtype=torch.float64, requires_grad=True)
    tf = torch.tensor(feat, dtype=torch.float64)
    ys = tf[torch.tensor(np.repeat(src, n))] @ tW.T
    yt = tf[torch.tensor(tgt.reshape(-1))] @ tW.T
    a, b = torch.nn.functional.normalize(ys, dim=-1), torch.nn.functional.normalize(yt, dim=-1)
    x = ((a * b).sum(-1) * tls.exp()).reshape(nq, n)
    x.retain_grad()
    pos = torch.argsort(x.detach(), dim=1, descending=True, stable=True)
    order = torch.empty_like(pos)
    order.scatter_(1, pos, torch.arange(1, n + 1).repeat(nq, 1))
    disc = 1.0 / torch.log2(1.0 + order.to(torch.float64))
    y = torch.tensor(rel, dtype=torch.float64)
    dy = y[:, :, None] - y[:, None, :]
    c = ((disc[:, :, None] - disc[:, None, :]) * dy).abs() * (dy > 0)
    lq = (c * -torch.nn.functional.logsigmoid(x[:, :, None] - x[:, None, :])).sum(dim=(1, 2))   # (softplus goes linear beyond 20)
    tw = torch.tensor(w, dtype=torch.float64)
    loss = (lq * tw).sum() / tw.sum()
    loss.backward()
    return float(loss.detach()), x.detach().numpy(), x.grad.numpy(), tW.grad.numpy(), float(tls.grad)


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / max(np.linalg.norm(b), 1e-300))


_LTR_SHAPES = [(1, 1), (3, 2), (5, 3), (7, 65), (2, 257)]


@pytest.mark.parametrize("nq,n", _LTR_SHAPES)
def test_oracle_gradients_against_autograd(nq, n):
    p = _ltr_problem(nq, n, seed=nq * 1000 + n)
    ref = _ltr_autograd(*p)
    got = sn.forward_backward(*p)
    by_id = sn.forward_backward_by_id(*p, sn.ranks(got[1]))
    if n == 1:   # no pair: everything is exactly 0
        for r in (ref, got, by_id):
            assert r[0] == 0.0 and r[4] == 0.0 and not np.any(r[2]) and not np.any(r[3])
        assert _rel(got[1], ref[1]) <= 1e-12 and _rel(by_id[1], got[1]) <= 1e-12
        return
    assert all(len(set(r)) >= 2 for r in p[5])   # every list has a pair
    for cand, base, tag in ((got, ref, "oracle vs autograd"), (by_id, got, "by_id vs oracle")):
        errs = {"loss": abs(cand[0] - base[0]) / abs(base[0]), "x": _rel(cand[1], base[1]), "dldx": _rel(cand[2], base[2]),
                "dW": _rel(cand[3], base[3]), "dls": abs(cand[4] - base[4]) / abs(base[4])}
        print(tag, (nq, n), {k: f"{e:.1e}" for k, e in errs.items()})
        for k, e in errs.items():
            assert e <= 1e-12, (tag, k, e)


def test_oracle_clamp_branch_against_autograd():
    """a target whose encoder output is exactly zero (feature row e_0, column 0 of W zero) while its feature row is not: F.normalize
    divides by the constant 1e-12 there, and dW's column 0 carries that row's dY / 1e-12"""
    nq, n = 3, 5
    feat, W, ls, src, tgt, rel, w = _ltr_problem(nq, n, seed=77)
    zid = int(np.setdiff1d(np.arange(feat.shape[0]), np.concatenate([src, tgt.reshape(-1)]))[0])
    tgt[1, 2] = zid
    feat[zid] = 0.0
    feat[zid, 0] = 1.0
    W[:, 0] = 0.0
    rel[1] = [0.0, 2.0, 4.0, 0.0, 1.0]
    p = (feat, W, ls, src, tgt, rel, w)
    ref = _ltr_autograd(*p)
    got = sn.forward_backward(*p)
    by_id = sn.forward_backward_by_id(*p, sn.ranks(got[1]))
    where = np.argwhere(tgt == zid)
    for r in (ref, got, by_id):
        assert all(r[1][q, j] == 0.0 for q, j in where)
    g = max(abs(ref[2][q, j]) for q, j in where)
    assert g > 0 and np.abs(ref[3][:, 0]).max() > 1e10 * g     # column 0 is ~ 1e12 dL/dx
    for cand, base, tag in ((got, ref, "oracle vs autograd"), (by_id, got, "by_id vs oracle")):
        errs = {"loss": abs(cand[0] - base[0]) / abs(base[0]), "dldx": _rel(cand[2], base[2]), "dW col 0": _rel(cand[3][:, 0], base[3][:, 0]),
                "dW rest": _rel(cand[3][:, 1:], base[3][:, 1:]), "dls": abs(cand[4] - base[4]) / abs(base[4])}
        print(tag, {k: f"{e:.1e}" for k, e in errs.items()})
        for k, e in errs.items():
            assert e <= 1e-12, (tag, k, e)


def _pairs(seed=0, v=50, rows=400):
    rng = np.random.default_rng(seed)
    return {"cliptype": rng.integers(0, 2, rows), "source_matchedid": rng.integers(0, 8, rows),
            "source_popularity": rng.choice([4.0, 9.0], rows), "target_matchedid": rng.integers(0, v, rows),
            "score": rng.integers(1, 4, rows).astype(np.float64)}   # (repeated scores: the sort must be stable)


def test_grouping_and_stable_sort():
    p = _pairs()
    tm = np.random.default_rng(1).random((50, 50)) < 0.3
    for split in ("training", "test"):
        got = sim.group_queries(p, tm, split)
        ref = sn.group_queries(list(p["cliptype"]), list(p["source_matchedid"]), list(p["source_popularity"]), list(p["target_matchedid"]),
                               list(p["score"]), tm, split)
        assert got == ref and len(got) > 4


class _StubModel:
    """hands out fixed hard negatives: ascending ids n - 1 .. 0 offset by the source"""
    def hard_negatives(self, split, sources, positives, n):
        self.calls = (split, list(sources), [list(x) for x in positives], n)
        return np.stack([np.arange(n, dtype=np.int32) + 100 * s for s in sources])


def test_positive_caps_and_list_assembly():
    n = 20
    cfg = sim.training_config({0: 50}, items_per_query=n)
    rows = 30   # one query with 30 positives, one with 3
    p = {"cliptype": np.zeros(rows + 3, int), "source_matchedid": np.array([1] * rows + [2] * 3),
         "source_popularity": np.array([16.0] * rows + [25.0] * 3), "target_matchedid": np.arange(rows + 3) % 50,
         "score": np.arange(rows + 3, dtype=np.float64)}
    tm = np.zeros((50, 50), bool)
    tr = sim.LTRDataset("training", cfg, p, tm, _StubModel())
    assert tr.max_num_positives == int(n * 0.9) == 18
    assert sim.training_config({0: 1})["items_per_query"] == 2048 and int(round(2048) * 0.9) == 1843
    d0 = tr[0]
    assert d0["targetid"].shape == (n,) and (d0["sourceid"] == 1).all() and d0["weight"][0] == 4.0
    assert list(d0["relevance"][:18]) == sorted(p["score"][:rows], reverse=True)[:18]
    assert list(d0["targetid"][18:]) == [100 + 18, 100 + 19]   # the last n - #pos of the ascending negatives
    d1 = tr[1]
    assert list(d1["targetid"][:3]) == [32, 31, 30] and list(d1["targetid"][3:]) == list(range(200 + 3, 200 + 20))
    assert (d1["relevance"][3:] == 0).all()
    tm[:, :] = True
    te = sim.LTRDataset("test", cfg, p, tm, _StubModel())
    assert te.max_num_positives == n and len(te[0]["targetid"]) == n
    b = next(tr.batches(2))
    assert b["targetid"].shape == (2, n) and b["weight"].shape == (2, 1)


def test_inf_fill_rule():
    # fewer admissible ids than n: np.argsort(kind="stable")[-n:] puts the largest inadmissible ids first, ascending
    w = np.array([0.5, 0.1, 0.9, 0.3, 0.3, 0.7])
    mask = np.array([False, True, False, True, True, False])
    got = sn.hard_negatives(w, 0, mask, "test", [], 5)
    assert list(got) == [2, 5, 1, 3, 4]   # admissible under "test" = mask: 1 (0.1), 3, 4 (0.3 tie, ascending id); fill: 2, 5
    got = sn.hard_negatives(w, 5, mask, "training", [2], 4)
    assert list(got) == [3, 4, 5, 0]      # admissible: 0 (0.5); fill: largest inadmissible ids 3, 4, 5 ascending
    tie = sn.hard_negatives(np.ones(6), 0, np.zeros(6, bool), "training", [], 3)
    assert list(tie) == [3, 4, 5]         # ties keep the larger ids, listed ascending


def test_early_stopper_and_csv(tmp_path):
    st = sim.EarlyStopper(patience=2, rtol=0.1)
    seq = []
    for score in (1.0, 0.95, 0.8, 0.85, 0.79):
        st(score)
        seq.append((st.save_model, st.stop, st.counter))
        if st.stop:
            break
    assert seq == [(True, False, 0), (True, False, 1), (True, False, 0), (False, False, 1), (True, True, 2)]

    class M:
        medium = 1

        def state_dict(self):
            return {"logit_scale": np.float32(2.5), "encoder.1.weight": np.ones((2, 3), np.float32)}

    sim.checkpoint_model(M(), -1, 0.5, 0.6, True, str(tmp_path), 1)
    sim.checkpoint_model(M(), 0, 0.4, 0.7, False, str(tmp_path), 1)
    rows = open(tmp_path / "pairwise.model.1.csv").read().splitlines()
    assert rows == ["epoch,training_loss,test_loss,saved", "-1,0.5,0.6,1", "0,0.4,0.7,0"]
    ck = sim.load_checkpoint(str(tmp_path / "pairwise.model.1.npz"))
    assert ck["encoder.1.weight"].shape == (2, 3) and float(ck["epoch"]) == -1


def test_cross_medium_map_recovers_a_rotation():
    rng = np.random.default_rng(2)
    d = 16
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    A = rng.standard_normal((40, d))
    B = A @ Q.T                               # B[i] = Q A[i]
    ids = np.arange(40)
    M = sim.cross_medium_map(A, B, ids, ids)
    np.testing.assert_allclose(M, Q, atol=1e-10)
    np.testing.assert_allclose(M, sn.closest_orthogonal_map(A.T, B.T), atol=1e-12)
    assert sim.avg_norm(M @ A.T - B.T) < 1e-20


def test_item_similarity_tables_layout():
    rng = np.random.default_rng(3)
    emb = {0: rng.standard_normal((30, 8)).astype(np.float32), 1: rng.standard_normal((20, 8)).astype(np.float32)}
    ad = {0: {"training": (np.arange(10), np.arange(10)), "test": (np.arange(10, 12), np.arange(10, 12))},
          1: {"training": (np.arange(10), np.arange(10)), "test": ([], [])}}
    t, metrics = sim.item_similarity_tables(emb, ad)
    assert set(t) == {"embeddings.0", "embeddings.1", "crossproject.0", "crossproject.1"}
    assert t["embeddings.0"].shape == (8, 30) and t["embeddings.1"].shape == (8, 20) and t["crossproject.0"].shape == (8, 8)
    np.testing.assert_array_equal(t["embeddings.0"], emb[0].T)
    M = t["crossproject.0"].astype(np.float64)
    np.testing.assert_allclose(M @ M.T, np.eye(8), atol=1e-5)
    assert set(metrics) == {"0.project.training", "0.project.test", "1.project.training", "1.project.test"}


def test_pack_testmask_bits():
    rng = np.random.default_rng(4)
    m = rng.random((37, 37)) < 0.5
    b = sim.pack_testmask(m).view(np.uint32)
    assert b.shape == (37, 2)
    for i in range(37):
        for j in range(37):
            assert bool((b[i, j >> 5] >> (j & 31)) & 1) == m[i, j]


def test_read_pairs_csv(tmp_path):
    fn = tmp_path / "pairs.0.csv"
    fn.write_text("cliptype,source_matchedid,source_popularity,target_matchedid,score\n1,3,4.0,5,0.5\n0,2,9,7,1.5\n")
    p = sim.read_pairs_csv(str(fn))
    assert list(p["cliptype"]) == [1, 0] and list(p["target_matchedid"]) == [5, 7] and list(p["score"]) == [0.5, 1.5]
