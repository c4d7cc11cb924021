"""GPU: windowed retrieval (rsys_retrieve_window): the ranks [start, start + len) of rsys_retrieve_request's ordering and the
exact admissible count, for groups with any number of queries including none.  Windows are checked byte for byte against slices of
rsys_retrieve_request where that call reaches (k = V_m <= 8192), as a strictly ordered permutation of the admissible set past its cap,
and exactly against an int64 oracle on integer-valued tables for groups without queries (tests/_render_items_np.py).  These are the
windows of whole requests; the windowed selection kernels alone (win_*_kernel through rsys_op_topk_window) are checked exactly, branch
by branch, on score populations built for them in tests/test_gpu_retrieve_select.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_items_np as ri  # noqa: E402
import _render_retrieval_np as rr  # noqa: E402

pytestmark = pytest.mark.gpu

DIM = 64
ERR_ARG = -1                     # RSYS_ERR_ARG
BIG = (9500, 2000)


def _model(dtype, vocab, seed=9):
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config("hd64", mask_rate=0.2, mask_topk=16)
    cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"] = vocab
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=4)
    model.init_weights(seed)
    model.random_pretrained_embeddings(seed + 1)
    return cfg, model


def _similarity(rng, V, dim=DIM):
    sim = {f"embeddings.{m}": (0.3 * rng.standard_normal((dim, V[m]))).astype(np.float32) for m in (0, 1)}
    sim.update({f"crossproject.{m}": (rng.standard_normal((dim, dim)) / np.sqrt(dim)).astype(np.float32) for m in (0, 1)})
    return sim


def _args(states, m, D, seed):
    from recommendersystem_amd import serve
    rng = np.random.default_rng(seed)
    for st in states:
        for u in st["users"]:
            u.setdefault("embeds", {f"{m}.retrieval": rng.standard_normal(D).astype(np.float32)})
    return serve.request_arrays(states, m)


def _check_padding(ids, scores, counts):
    for g in range(ids.shape[0]):
        assert (ids[g, counts[g]:] == -1).all() and np.isneginf(scores[g, counts[g]:]).all()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_window_equals_slice(dtype):
    from recommendersystem_amd import serve
    V = (3000, 2000)
    cfg, model = _model(dtype, V)
    rng = np.random.default_rng(21)
    rel = rr.random_relations(rng, V, density=0.0005)
    sim = _similarity(rng, V)
    released = {m: rng.random(V[m]) < 0.9 for m in (0, 1)}
    serve.load_retrieval_tables(model, rel, sim, released)
    for m in (0, 1):
        states = [rr.random_state(rng, V, m, n_users=1 + j % 3, n_items=50, n_selected=j % 4) for j in range(6)]
        q, group, hist, sel = _args(states, m, cfg["embed_dim"], 30 + m)
        full_ids, full_sc, full_cnt = model.retrieve_request(q, m, V[m], group=group, histories=hist, selected=sel)
        total = np.array([int((~rr.set_mask(m, rel, st, V, released=released[m])).sum()) for st in states])
        assert np.array_equal(full_cnt, total)
        for start, length in ((0, 1), (0, 1024), (1000, 1024), (total - 5, 1024), (total, 7), (total + 100, 1)):
            starts = np.broadcast_to(np.asarray(start, np.int64), (6,))
            ids, sc, cnt, tot = model.retrieve_window(q, m, starts, [length] * 6, group=group, histories=hist, selected=sel)
            assert np.array_equal(tot, total)
            assert np.array_equal(cnt, np.clip(total - starts, 0, length))
            _check_padding(ids, sc, cnt)
            for g in range(6):
                s0, n = int(starts[g]), int(cnt[g])
                assert ids[g, :n].tobytes() == full_ids[g, s0:s0 + n].tobytes(), (m, g, start, length)
                assert sc[g, :n].tobytes() == full_sc[g, s0:s0 + n].tobytes(), (m, g, start, length)
    model.close()


@pytest.fixture(scope="module")
def big():
    """hd64 model with V = (9500, 2000): random relations, INTEGER similarity tables (tests/_render_items_np.py), a released mask"""
    from recommendersystem_amd import serve
    cfg, model = _model("fp32", BIG)
    rng = np.random.default_rng(22)
    rel = {}
    for m in (0, 1):        # a few hundred entries per table: the rules mask some hundred items, more than 8192 of medium 0 stay admissible
        rel[f"{m}.dependencies"] = rr.random_csc(rng, BIG[m], BIG[m], 300.0 / BIG[m] ** 2)
        rel[f"{m}.recaps"] = rr.random_csc(rng, BIG[m], BIG[m], 200.0 / BIG[m] ** 2)
        rel[f"{m}.adaptations"] = rr.random_csc(rng, BIG[m], BIG[1 - m], 300.0 / (BIG[0] * BIG[1]))
    sim, which = ri.integer_tables(rng, BIG)
    released = {m: rng.random(BIG[m]) < 0.97 for m in (0, 1)}
    serve.load_retrieval_tables(model, rel, sim, released)
    yield dict(cfg=cfg, model=model, rel=rel, sim=sim, which=which, released=released)
    model.close()


def test_past_the_cap(big):
    model, V, m = big["model"], BIG, 0
    rng = np.random.default_rng(23)
    states = [rr.random_state(rng, V, m, n_users=1 + j, n_items=80, n_selected=j) for j in range(3)]
    q, group, hist, sel = _args(states, m, big["cfg"]["embed_dim"], 31)
    cap_ids, cap_sc, cap_cnt = model.retrieve_request(q, m, 8192, group=group, histories=hist, selected=sel)
    adm = [np.flatnonzero(~rr.set_mask(m, big["rel"], st, V, released=big["released"][m])) for st in states]
    assert all(a.size > 8192 for a in adm) and (cap_cnt == 8192).all()
    got_ids, got_sc = [[] for _ in states], [[] for _ in states]
    for start in range(0, max(a.size for a in adm), 1024):
        ids, sc, cnt, tot = model.retrieve_window(q, m, [start] * 3, [1024] * 3, group=group, histories=hist, selected=sel)
        _check_padding(ids, sc, cnt)
        for g in range(3):
            assert tot[g] == adm[g].size and cnt[g] == min(max(adm[g].size - start, 0), 1024)
            got_ids[g].append(ids[g, :cnt[g]]); got_sc[g].append(sc[g, :cnt[g]])
    for g in range(3):
        ids, sc = np.concatenate(got_ids[g]), np.concatenate(got_sc[g])
        assert np.array_equal(np.sort(ids), adm[g])                                   # a permutation of the admissible set
        assert ids[:8192].tobytes() == cap_ids[g].tobytes() and sc[:8192].tobytes() == cap_sc[g].tobytes()
        d = np.diff(sc)
        assert (d <= 0).all() and (np.diff(ids)[d == 0] > 0).all()                    # (score, id) strictly ordered


def _bare(m, sel):
    return dict(medium=m, users=[], items=[dict(medium=a, matchedid=int(i)) for a, i in sel])


def _bare_states(big, m):
    """user-less states: a same-medium selection, a cross-medium one, a duplicate, none, one that sums to the zero vector"""
    w = big["which"][m]
    plus, minus = np.flatnonzero(w == 0), np.flatnonzero(w == 1)
    return [_bare(m, [(m, 17), (m, 4000 % BIG[m])]), _bare(m, [(1 - m, 23), (m, 99)]), _bare(m, [(m, 301), (m, 301), (1 - m, 5)]),
            _bare(m, []), _bare(m, [(m, plus[3]), (m, minus[3])])]


@pytest.mark.parametrize("m", [0, 1])
def test_user_less_groups_are_exact(big, m):
    model = big["model"]
    states = _bare_states(big, m)
    sel = [[(a["medium"], a["matchedid"]) for a in st["items"]] for st in states]
    want = [ri.ordering_exact(m, big["sim"], st, BIG, big["released"][m]) for st in states]
    assert np.array_equal(want[3][0], np.flatnonzero(big["released"][m][1:]) + 1)         # no selection: ascending id
    assert not want[4][1].any() and not want[3][1].any()                                  # the zero vector: +0.0 everywhere
    # where the scores change (tie-block edges) in the first state's ordering: windows inside a block, across one, to the end
    edges = np.flatnonzero(np.diff(want[0][1])) + 1
    assert edges.size >= 2 and np.diff(np.concatenate([[0], edges])).max() >= 300         # blocks of hundreds of items
    e = int(edges[0])
    windows = [(0, 1), (e // 2, 100) if e >= 200 else (0, 50), (max(e - 3, 0), 10), (e - 500 if e > 500 else 0, 1024), (e, 1024), (0, 1024)]
    for start, length in windows:
        starts = [start] * len(states)
        ids, sc, cnt, tot = model.retrieve_window(None, m, starts, [length] * len(states), selected=sel)
        _check_padding(ids, sc, cnt)
        for g, (wid, wsc) in enumerate(want):
            n = min(max(wid.size - start, 0), length)
            assert tot[g] == wid.size and cnt[g] == n
            assert np.array_equal(ids[g, :n], wid[start:start + n]), (g, start, length)
            assert sc[g, :n].tobytes() == wsc[start:start + n].tobytes(), (g, start, length)
    # ending at the total, per group
    starts = [w[0].size - 700 for w in want]
    ids, sc, cnt, tot = model.retrieve_window(None, m, starts, [1024] * len(states), selected=sel)
    for g, (wid, wsc) in enumerate(want):
        assert cnt[g] == 700 and np.array_equal(ids[g, :700], wid[-700:]) and sc[g, :700].tobytes() == wsc[-700:].tobytes()


def test_mixed_call_equals_each_group_alone(big):
    model, m = big["model"], 0
    rng = np.random.default_rng(24)
    with_users = [rr.random_state(rng, BIG, m, n_users=2, n_items=60, n_selected=2), rr.random_state(rng, BIG, m, n_users=1, n_items=60, n_selected=0)]
    q, _, hist, sel_u = _args(with_users, m, big["cfg"]["embed_dim"], 32)
    bare = _bare_states(big, m)[:2]
    sel_b = [[(a["medium"], a["matchedid"]) for a in st["items"]] for st in bare]
    # groups: bare 0, users 0 (two queries), bare 1, users 1 (one query)
    group = np.array([1, 1, 3], np.int32)
    sel = [sel_b[0], sel_u[0], sel_b[1], sel_u[1]]
    starts, lens = [0, 5000, 8800, 1000], [1024, 1024, 1024, 300]
    mixed = model.retrieve_window(q, m, starts, lens, group=group, n_groups=4, histories=hist, selected=sel)
    alone = [model.retrieve_window(None, m, [starts[0]], [lens[0]], selected=[sel[0]]),
             model.retrieve_window(q[:2], m, [starts[1]], [lens[1]], group=[0, 0], histories=hist[:2], selected=[sel[1]]),
             model.retrieve_window(None, m, [starts[2]], [lens[2]], selected=[sel[2]]),
             model.retrieve_window(q[2:], m, [starts[3]], [lens[3]], group=[0], histories=hist[2:], selected=[sel[3]])]
    for g, one in enumerate(alone):
        for x, y in zip(mixed, one):
            assert x[g].tobytes() == y[0].tobytes(), g
    assert mixed[2][0] == 1024 and mixed[2][1] == 1024 and mixed[2][3] == 300
    again = model.retrieve_window(q, m, starts, lens, group=group, n_groups=4, histories=hist, selected=sel)
    for x, y in zip(mixed, again):
        assert x.tobytes() == y.tobytes()                                             # bitwise reproducible


def test_argument_errors_leave_outputs_untouched():
    import recommendersystem_amd as ra
    V = (3000, 2000)
    cfg, model = _model("fp32", V)
    L = ra.lib()
    q = np.random.default_rng(25).standard_normal((2, cfg["embed_dim"])).astype(np.float32)

    def call(starts, lens, sel=None, nq=0):
        ng = len(starts)
        ws, wl = np.asarray(starts, np.int64), np.asarray(lens, np.int32)
        bufs = [np.full((ng, 1024), 0x5A5A5A5A, np.int32), np.full((ng, 1024), 0x5A5A5A5A, np.int32).view(np.float32),
                np.full(ng, 0x5A5A5A5A, np.int32), np.full(ng, 0x5A5A5A5A, np.int32)]
        sp = (None, None, None)
        if sel is not None:
            off = np.zeros(ng + 1, np.int64); off[1:] = np.cumsum([len(s) for s in sel])
            flat = np.asarray([a for s in sel for a in s], np.int32).reshape(-1, 2)
            keep = (off, np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1]))
            sp = tuple(a.ctypes.data for a in keep)
        rc = L.rsys_retrieve_window(model._h, 0, q.ctypes.data if nq else None, nq, None, ng, None, None, None, None, *sp, ws.ctypes.data,
                                    wl.ctypes.data, *(b.ctypes.data for b in bufs))
        clean = all((b.view(np.int32) == 0x5A5A5A5A).all() for b in bufs)
        return rc, clean

    assert call([0, 0], [10, 10]) == (0, False)                                       # a good call writes its outputs
    for starts, lens in (([0, 0], [10, 0]), ([0, 0], [1025, 10]), ([0, -1], [10, 10])):
        rc, clean = call(starts, lens)
        assert rc == ERR_ARG and clean, (starts, lens)
    rc, clean = call([0, 0], [10, 10], sel=[[(0, 5)], []])                            # selected items, no similarity table
    assert rc == ERR_ARG and clean
    rc, clean = call([0, 0], [10, 10], nq=2)                                          # queries without the relation tables
    assert rc == ERR_ARG and clean
    with pytest.raises(ra.RsysError):
        model.retrieve_window(None, 0, [0], [0])
    model.close()
