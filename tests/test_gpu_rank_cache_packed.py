"""GPU: ranking on packed rows through the K/V cache (rsys_rank_cache_store_packed / _candidates_packed, serve.predict_ranking_full(pack=True);
DESIGN 4zd) on the whole model, plain and four-adapter bank, fp32 and bf16: the packed request against the one-user-per-row request, the
slots a packed store fills against the row store's, isolation between the users of one packed forward, the fp64 oracle on the reference's
row, the refusals, and no side effect on training."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _adapter_bank_util as ab  # noqa: E402
import _trim_util as tu  # noqa: E402
import test_gpu_rank_cache as trc  # noqa: E402

pytestmark = pytest.mark.gpu

# the hd64 dimensions at max_sequence_length 128 (tests/_trim_util.config), max_rows 4

N_HIST = [1, 4, 31, 32, 33, 60, 127]          # S = 128: one event, inside a tile, around a tile boundary, two tiles, S - 1
KINDS = [("base", "fp32"), ("base", "bf16"), ("bank", "fp32"), ("bank", "bf16")]


def _users(rng, V, S, medium):
    """the seven histories with 1 / 3 / 33 / S + 5 candidates in turn, a user with an empty history and one without candidates"""
    n_cand = [1, 3, 33, S + 5, 3, 33, 1]
    users = [trc.make_user(rng, nh, rng.integers(1, V[medium], size=nc), V) for nh, nc in zip(N_HIST, n_cand)]
    users.insert(2, trc.make_user(rng, 0, rng.integers(1, V[medium], size=4), V))
    users.insert(5, trc.make_user(rng, 20, [], V))
    return users


def _store_rows(cfg, V, users, placed):
    """packed store rows: placed = [(user index, row, first_column, slot)] -> (d, segments)"""
    from recommendersystem_amd import serve
    S = cfg["max_sequence_length"]
    d = serve._empty_rows(1 + max(p[1] for p in placed), S)
    seg = []
    for k, (u, row, c0, slot) in enumerate(placed):
        h = serve._history(users[u], S)
        serve._fill_row(d, row, h, len(h), users[u]["user"], V[0], False, c0)
        d["userid"][row, c0:c0 + len(h)] = k + 1
        seg.append((row, c0, len(h), slot))
    return d, seg


def _cand_rows(cfg, V, users, medium, placed):
    """packed candidate rows: placed = [(user index, row, first_column, first candidate, candidates, slot)] -> (d, segments)"""
    from recommendersystem_amd import serve
    S = cfg["max_sequence_length"]
    d = serve._empty_rows(1 + max(p[1] for p in placed), S)
    seg = []
    for u, row, c0, first, n, slot in placed:
        seq = [serve.make_item(users[u]["timestamp"], medium, c) for c in users[u]["ranking_items"][first:first + n]]
        serve._fill_row(d, row, seq, 0, users[u]["user"], V[0], False, c0)
        seg.append((row, c0, n, slot))
    return d, seg


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_packed_request_equals_the_row_request(kind, dtype):
    """predict_ranking_full(pack=True) == pack=False, value for value: the kernels share their bodies with the row forms, the trunk is
    token-local outside attention, and at this size trimming and packing measured a difference of exactly 0.0."""
    from recommendersystem_amd import serve
    cfg, V = tu.config()
    S = cfg["max_sequence_length"]
    model, _, _ = trc._model(cfg, kind, dtype)
    for medium in (0, 1):
        users = _users(np.random.default_rng(21 + medium), V, S, medium)
        rows = serve.predict_ranking_full(model, users, medium)
        packed = serve.predict_ranking_full(model, users, medium, pack=True)
        key = f"{medium}.ranking"
        assert [len(p[key]) for p in packed] == [len(u["ranking_items"]) for u in users]
        diff = max(float(np.abs(np.asarray(a[key]) - np.asarray(b[key])).max()) for a, b in zip(rows, packed) if a[key])
        print(f"packed vs rows {kind} {dtype} medium {medium}: max |difference| {diff:.3e}")
        assert packed == rows
        # fewer slots than users: more waves, the same values
        assert serve.predict_ranking_full(model, users, medium, pack=True, cache_slots=3) == rows
    model.close()


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_packed_store_fills_the_slots_the_row_store_fills(kind, dtype):
    """rank_cache_get of every layer and slot after the plan's packed store forwards == after rank_cache_store of the same histories, one
    per row"""
    from recommendersystem_amd import serve
    cfg, V = tu.config()
    S, L = cfg["max_sequence_length"], cfg["num_layers"]
    model, _, _ = trc._model(cfg, kind, dtype)
    rng = np.random.default_rng(33)
    users = [trc.make_user(rng, nh, [1], V) for nh in N_HIST] + [trc.make_user(rng, 127, [1], V)]
    n = len(users)
    adapter = ab.SLOT_MAP["1.ranking"] if kind == "bank" else None
    model.rank_cache_reserve(2 * n)
    for u0 in range(0, n, 4):
        dh, nh = trc._hist_rows(cfg, users[u0:u0 + 4], V)
        model.rank_cache_store(dh, nh, list(range(u0, u0 + len(nh))), adapters=adapter)
    (stores, _), = serve.rank_cache_pack_plan([len(u["items"]) for u in users], [1] * n, S, model.max_rows, n)
    assert len(stores) == 1 and any(p[2] for p in stores[0][1])          # one packed forward instead of two
    for row_len, placed in stores:
        d, seg = _store_rows(cfg, V, users, [(u, row, c0, n + slot) for u, row, c0, _, slot in placed])
        model.rank_cache_store_packed(d, seg, adapters=adapter, row_len=row_len)
    for u in range(n):
        for l in range(L):
            assert np.array_equal(model.rank_cache_get(l, u, len(users[u]["items"])), model.rank_cache_get(l, n + u, len(users[u]["items"]))), (u, l)
    model.close()


def test_first_packed_forward_of_a_fresh_bank_model():
    """The first per-tile binding of a model allocates the bank's tile map; its zero fill must not land on the map that is copied into it
    (every tile then ran slot 0).  A fresh bank model at the hd64 configuration's own S = 64: four short histories at row_len 32 as its
    first packed call, then the row store of the same histories into other slots -- every layer of every slot equal."""
    cfg, V = trc._cfg("hd64")
    L = cfg["num_layers"]
    model, _, _ = trc._model(cfg, "bank", "fp32")
    rng = np.random.default_rng(6)
    users = [trc.make_user(rng, nh, [1], V) for nh in (1, 4, 31, 32)]
    model.rank_cache_reserve(8)
    d, seg = _store_rows(cfg, V, users, [(u, u, 0, u) for u in range(4)])
    model.rank_cache_store_packed(d, seg, adapters=1, row_len=32)
    dh, nh = trc._hist_rows(cfg, users, V)
    model.rank_cache_store(dh, nh, [4, 5, 6, 7], adapters=1)
    assert all(np.array_equal(model.rank_cache_get(l, u, nh[u]), model.rank_cache_get(l, 4 + u, nh[u])) for u in range(4) for l in range(L))
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_users_of_one_packed_forward_do_not_see_each_other(dtype):
    """A (33 events, 5 candidates), B (4, 3) and C (31, 33) share one store forward and one candidate forward, A and B a row of each.
    Replacing B's history, its candidates or its adapter slot leaves A's and C's values bit-identical and moves B's."""
    cfg, V = tu.config()
    model, _, _ = trc._model(cfg, "bank", dtype)
    model.rank_cache_reserve(4)
    rng = np.random.default_rng(8)
    A = trc.make_user(rng, 33, rng.integers(1, V[0], size=5), V)
    B = trc.make_user(rng, 4, rng.integers(1, V[0], size=3), V)
    C = trc.make_user(rng, 31, rng.integers(1, V[0], size=33), V)
    B_hist = dict(trc.make_user(rng, 7, [], V), ranking_items=B["ranking_items"])
    B_cand = dict(B, ranking_items=[1 + (c + 5) % (V[0] - 1) for c in B["ranking_items"]])

    def run(b, b_slot):
        users = [A, b, C]
        ad = [1, b_slot, 3]
        d, seg = _store_rows(cfg, V, users, [(0, 0, 0, 2), (1, 0, 64, 0), (2, 1, 0, 1)])
        model.rank_cache_store_packed(d, seg, adapters=ad, row_len=128)
        d, seg = _cand_rows(cfg, V, users, 0, [(0, 0, 0, 0, 5, 2), (1, 0, 32, 0, 3, 0), (2, 1, 64, 0, 33, 1)])
        v = model.rank_cache_candidates_packed(d, seg, adapters=ad, row_len=128)
        assert v.shape == (41,) and np.isfinite(v).all()
        return v[:5], v[5:8], v[8:]

    a0, b0, c0 = run(B, 1)
    for b, slot in ((B_hist, 1), (B_cand, 1), (B, 2), (B, -1)):
        a1, b1, c1 = run(b, slot)
        assert np.array_equal(a0, a1) and np.array_equal(c0, c1)
        assert not np.array_equal(b0, b1)
    # the same segments placed elsewhere: other rows, other tiles, another order, A's list cut in two
    users = [A, B, C]
    d, seg = _store_rows(cfg, V, users, [(2, 0, 0, 1), (1, 1, 32, 0), (0, 1, 64, 2)])
    model.rank_cache_store_packed(d, seg, adapters=[3, 1, 1], row_len=128)
    d, seg = _cand_rows(cfg, V, users, 0, [(1, 1, 96, 0, 3, 0), (0, 0, 64, 3, 2, 2), (2, 1, 0, 0, 33, 1), (0, 0, 0, 0, 3, 2)])
    v = model.rank_cache_candidates_packed(d, seg, adapters=[1, 1, 3, 1], row_len=128)
    # (forwards of the same two rows, so the same GEMM route; a token's sums do not depend on where in the batch it sits)
    moved = max(trc.relerr(v[:3], b0), trc.relerr(np.concatenate([v[38:], v[3:5]]), a0), trc.relerr(v[5:38], c0))
    print(f"segments placed elsewhere, {dtype}: largest relative difference {moved:.3e}")
    assert np.array_equal(v[:3], b0) and np.array_equal(np.concatenate([v[38:], v[3:5]]), a0) and np.array_equal(v[5:38], c0)
    model.close()


@pytest.mark.parametrize("kind", ["base", "bank"])
def test_packed_path_against_the_oracle(kind):
    """fp32: a user with S - 1 events and S candidates beside a short user, through the packed path, within 1e-4 of
    OracleModel(max_sequence_length = 2S, float64) on the reference's row"""
    from recommendersystem_amd import serve
    cfg, V = tu.config()
    S = cfg["max_sequence_length"]
    medium = 1
    rng = np.random.default_rng(5)
    user = trc.make_user(rng, S - 1, rng.choice(np.arange(1, V[medium]), size=S, replace=S > V[medium] - 1), V)
    short = trc.make_user(rng, 9, rng.integers(1, V[medium], size=7), V)
    model, P, adapters = trc._model(cfg, kind, "fp32")
    got = serve.predict_ranking_full(model, [short, user, short], medium, pack=True)
    for u, g in zip([short, user], got):
        ref = trc.oracle_full(cfg, P, adapters, kind, u, medium, V)
        err = trc.relerr(g[f"{medium}.ranking"], ref)
        print(f"packed path against the fp64 oracle, {kind}, {len(u['items'])} events, {len(u['ranking_items'])} candidates: {err:.3e}")
        assert err < 1e-4, err
    assert got[0] == got[2]
    model.close()


def test_refusals_leave_outputs_and_slots_untouched():
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import _lib
    Lb = _lib.lib()
    ARG = -1
    cfg, V = tu.config()
    S, L = cfg["max_sequence_length"], cfg["num_layers"]
    rng = np.random.default_rng(4)
    model, P, adapters = trc._model(cfg, "base", "fp32", max_rows=2)
    h = model._h
    out = np.full(16, 123.0, np.float32)

    def store(seg, ad=None):
        s = np.array(seg, np.int32).reshape(-1, 4); a = None if ad is None else np.array(ad, np.int32)
        return Lb.rsys_rank_cache_store_packed(h, None if a is None else a.ctypes.data, len(s), s.ctypes.data)

    def cands(seg, ad=None):
        s = np.array(seg, np.int32).reshape(-1, 4); a = None if ad is None else np.array(ad, np.int32)
        return Lb.rsys_rank_cache_candidates_packed(h, None if a is None else a.ctypes.data, len(s), s.ctypes.data, out.ctypes.data)

    assert store([(0, 0, 3, 0)]) == ARG                                               # nothing reserved
    model.rank_cache_reserve(4)
    assert store([(0, 0, 3, 0)]) == ARG and cands([(0, 0, 1, 0)]) == ARG              # no batch uploaded
    users = [trc.make_user(rng, 3, [1, 2], V), trc.make_user(rng, 5, [3], V), trc.make_user(rng, 40, [3], V)]
    d, good = _store_rows(cfg, V, users, [(0, 0, 0, 0), (1, 0, 32, 1), (2, 1, 0, 2)])
    model.upload(d)
    assert store([(0, 16, 3, 0)]) == ARG and store([(0, -32, 3, 0)]) == ARG           # a first column that is not a multiple of 32
    assert store([(0, 96, 33, 0)]) == ARG and store([(0, 128, 1, 0)]) == ARG          # across the row's end
    assert store([(2, 0, 3, 0)]) == ARG and store([(-1, 0, 3, 0)]) == ARG             # a row outside the batch
    assert store([(0, 0, 33, 0), (0, 32, 5, 1)]) == ARG                               # two segments on one tile
    assert store([(0, 0, S + 1, 0)]) == ARG and store([(0, 0, -1, 0)]) == ARG         # n_hist outside [0, S]
    assert store([(0, 0, 3, 1), (0, 32, 5, 1)]) == ARG                                # duplicate slots
    assert store([(0, 0, 3, 4)]) == ARG and store([(0, 0, 3, -1)]) == ARG             # a slot outside the reserve
    assert store(good, [0, -1, -1]) == ARG                                            # an adapter slot that is not complete (no bank)
    assert store(good, [9, -1, -1]) == ARG
    assert store([(0, 0, 1, 0)] * 9) == ARG and store([], None) == ARG                # more segments than tiles; none
    assert cands([(0, 0, 1, 0)]) == ARG                                               # never stored: every store above was refused
    with pytest.raises(ra.RsysError):
        model.rank_cache_get(0, 0, 3)
    assert store(good) == 0
    kv = [model.rank_cache_get(l, s, n) for l in range(L) for s, n in ((0, 3), (1, 5), (2, 40))]
    # refused stores that name stored slots leave them stored, with what they held
    assert store([(0, 0, 3, 0), (0, 48, 5, 1)]) == ARG and store([(0, 0, 3, 0), (0, 0, 5, 1)]) == ARG
    assert all(np.array_equal(a, b) for a, b in zip(kv, [model.rank_cache_get(l, s, n) for l in range(L) for s, n in ((0, 3), (1, 5), (2, 40))]))
    dc, cgood = _cand_rows(cfg, V, users, 0, [(0, 0, 0, 0, 2, 0), (1, 0, 32, 0, 1, 1), (2, 1, 64, 0, 1, 2)])
    model.upload(dc)
    assert cands([(0, 0, 1, 3)]) == ARG                                               # slot 3 never stored
    assert cands([(0, 0, 1, 4)]) == ARG                                               # outside the reserve
    assert cands([(0, 0, 0, 0)]) == ARG and cands([(0, 0, S + 1, 0)]) == ARG          # n_cand outside [1, S]
    assert cands([(0, 8, 1, 0)]) == ARG and cands([(0, 96, 33, 0)]) == ARG and cands([(2, 0, 1, 0)]) == ARG
    assert cands([(0, 0, 33, 0), (0, 32, 1, 1)]) == ARG                               # overlap
    assert cands(cgood, [-1, 5, -1]) == ARG                                           # an incomplete adapter slot
    assert np.all(out == 123.0)
    assert cands(cgood) == 0 and np.all(out[:4] != 123.0) and np.all(out[4:] == 123.0)
    # a slot that holds S events cannot serve candidates (they would sit at position S)
    full = trc.make_user(rng, S - 1, [1], V)
    dS, _ = trc._hist_rows(cfg, [full], V)
    model.upload(dS)
    assert store([(0, 0, S, 3)]) == 0
    model.upload(dc)
    out[:] = 123.0
    assert cands([(0, 0, 1, 3)]) == ARG and np.all(out == 123.0)
    model.close()
    # models the cache does not serve packed: fp8 and row-sharded (no reserve either), finetune = 1
    for kind in ("fp8", "sharded", "finetune"):
        if kind == "fp8":
            c8 = synth.make_config("f8t", mask_rate=0.2, mask_topk=16)
            m8 = ra.RecommenderModel(c8, dtype="fp8", max_rows=2)
        elif kind == "sharded":
            c8 = synth.make_config("tiny", mask_rate=0.2, mask_topk=4)
            c8["table_shard"] = (0, 1)
            m8 = ra.RecommenderModel(c8, dtype="fp32", max_rows=2)
        else:
            c8 = ab.finetune_config(cfg)
            m8 = ra.RecommenderModel(c8, dtype="fp32", max_rows=2)
            m8.load_state_dict(dict(P, **adapters[0]))
            assert Lb.rsys_rank_cache_reserve(m8._h, 2) == 0
            m8.upload(d)
        h = m8._h
        assert store([(0, 0, 3, 0)]) == ARG and cands([(0, 0, 1, 0)]) == ARG and np.all(out == 123.0), kind
        m8.close()


def test_a_partially_loaded_adapter_slot_is_refused():
    """A bank model whose slot 5 holds one tensor of an adapter: naming it for a segment is RSYS_ERR_ARG from the completeness check of the
    per-tile binding, for both calls; no slot is marked stored, `out` is untouched, and nothing stays bound -- the base-model calls
    that follow store and rank what the row calls do."""
    import recommendersystem_amd as ra
    from recommendersystem_amd import _lib
    Lb = _lib.lib()
    cfg, V = tu.config()
    L = cfg["num_layers"]
    model, _, adapters = trc._model(cfg, "bank", "fp32")
    name, shape = model.adapter_names()[0]
    one = np.ascontiguousarray(adapters[0][name], np.float32)
    assert Lb.rsys_adapter_set(model._h, 5, name.encode(), one.ctypes.data, one.size) == 0 and 5 not in model.adapters_loaded()
    rng = np.random.default_rng(14)
    users = [trc.make_user(rng, 9, [1, 2, 3], V), trc.make_user(rng, 33, [4], V)]
    model.rank_cache_reserve(4)
    d, seg = _store_rows(cfg, V, users, [(0, 0, 0, 0), (1, 0, 32, 1)])
    with pytest.raises(ra.RsysError):
        model.rank_cache_store_packed(d, seg, adapters=[1, 5])
    for slot in (0, 1):
        with pytest.raises(ra.RsysError):
            model.rank_cache_get(0, slot, len(users[slot]["items"]))      # never stored
    model.rank_cache_store_packed(d, seg)                                 # the base model on both segments
    dh, nh = trc._hist_rows(cfg, users, V)
    model.rank_cache_store(dh, nh, [2, 3])
    assert all(np.array_equal(model.rank_cache_get(l, u, nh[u]), model.rank_cache_get(l, 2 + u, nh[u])) for u in range(2) for l in range(L))
    dc, cseg = _cand_rows(cfg, V, users, 0, [(0, 0, 0, 0, 3, 0), (1, 0, 32, 0, 1, 1)])
    model.upload(dc)
    out = np.full(4, 123.0, np.float32)
    sg, ad = np.array(cseg, np.int32), np.array([5, 1], np.int32)
    assert Lb.rsys_rank_cache_candidates_packed(model._h, ad.ctypes.data, 2, sg.ctypes.data, out.ctypes.data) == -1 and np.all(out == 123.0)
    got = model.rank_cache_candidates_packed(dc, cseg)
    rows = model.rank_cache_candidates({k: np.concatenate([trc._cand_rows(cfg, u, 0, V, [(0, len(u["ranking_items"]))])[k] for u in users], 0) for k in dc},
                                       [2, 3], [3, 1])
    assert np.array_equal(got, rows)
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_packed_calls_between_training_steps_change_nothing(dtype):
    """Deterministic mode: step -> reserve + packed store + packed candidates -> step gives the step -> step results bit for bit."""
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config("hd64", mask_rate=0.2, deterministic=True, max_sequence_length=tu.S_TEST)
    V = (cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"])
    S = cfg["max_sequence_length"]
    P = synth.make_params(cfg, 3, "test")
    rows = 4
    batches = [synth.make_batch(cfg, rows, 40 + i) for i in range(2)]
    masks = [synth.make_masks(cfg, rows, 50 + i) for i in range(2)]
    names = synth.trainable_names(cfg)
    rng = np.random.default_rng(2)
    users = [trc.make_user(rng, 60, rng.integers(1, V[0], size=40), V), trc.make_user(rng, 5, rng.integers(1, V[0], size=9), V)]

    def run(with_cache):
        model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
        model.load_state_dict(P)
        opt = ra.create_optimizer(model, dict(cfg, learning_rate=1e-2))
        model.set_loss_weights(trc.TASK_W, 1)
        out = []
        for i, (d, mk) in enumerate(zip(batches, masks)):
            if i == 1 and with_cache:
                model.rank_cache_reserve(2)
                dh, seg = _store_rows(cfg, V, users, [(0, 0, 0, 1), (1, 0, 64, 0)])
                model.rank_cache_store_packed(dh, seg, row_len=96)
                dc, seg = _cand_rows(cfg, V, users, 0, [(0, 0, 0, 0, 40, 1), (1, 0, 64, 0, 9, 0)])
                vals = model.rank_cache_candidates_packed(dc, seg)
                assert np.isfinite(vals).all() and vals.size == 49
            out.append(np.array(model(d, False, masks=mk), np.float32))
            out += [model.grad(n).copy() for n in names]
            opt.step(clip_max_norm=1.0)
        out += [model.get_parameter(n).copy() for n in names]
        model.close()
        return out

    a, b = run(False), run(True)
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_render_users_with_packed_store_rows(kind, dtype):
    """render_users(full_history=True, pack=True, pack_ranking=True) against pack_ranking=False on the 5 states / 9 users of
    tests/test_gpu_packed_render.py, with eight cache slots reserved (one store wave instead of two): pages, totals and r_masked are equal,
    the library's forward counters are serve.render_full_forwards(pack_store=True)'s and its packed store forwards (rows, row_len) are
    serve.render_full_store_rows'."""
    import test_gpu_render_full as rf
    import test_gpu_render_request as rq
    from recommendersystem_amd import serve
    cfg, V = tu.config()
    model, _, _ = tu.make_model(cfg, kind, dtype, max_rows=4)
    try:
        S, RM = cfg["max_sequence_length"], model.max_rows
        rq._tables(model, V)
        states, pags, registry = rq._request()
        states[0]["users"][0]["user"]["items"] = []                        # a user with an empty history
        assert sum(len(st["users"]) for st in states) == 9 and len(states) == 5
        model.rank_cache_reserve(8)
        model.render_keep(True)
        assert model.serving_pack_ranking() is False                       # default off
        res, k, fr = {}, {}, {}
        for on in (False, True):
            res[on] = serve.render_users(model, states, pags, registry, full_history=True, pack=True, pack_ranking=on)
            k[on] = rf._kept(model, cfg, states)
            fr[on] = model.render_kept("forward_rows").reshape(-1, 3).copy()
            assert model.serving_pack_ranking() is False and model.serving_pack is False
        for (pa, ta), (pb, tb) in zip(res[False], res[True]):
            assert np.array_equal(pa, pb) and ta == tb
        d_r = float(np.abs(k[True]["r_masked"] - k[False]["r_masked"]).max())
        print(f"render pack_ranking {kind} [{dtype}]: max |packed - unpacked| r_masked {d_r:.3e}")
        assert np.array_equal(k[True]["r_masked"], k[False]["r_masked"]) and np.array_equal(k[True]["queries"], k[False]["queries"])
        _, cand_of = rf._windows(k[True], states, pags, res[True])
        _, _, nh, nc = rf._plan_inputs(k[True], cfg, states, cand_of)
        assert k[False]["full"].tolist() == list(serve.render_full_forwards(nh, nc, S, RM))
        want = serve.render_full_forwards(nh, nc, S, RM, pack_store=True, slots=8)
        assert k[True]["full"].tolist() == list(want), (k[True]["full"], want, nh, nc)
        store = fr[True][fr[True][:, 0] == 1][:, 1:].tolist()
        assert store == [list(x) for x in serve.render_full_store_rows(nh, S, RM, slots=8)]
        assert want[0] < k[False]["full"][0]                               # fewer store forwards
        # every user with a history is stored once, in the slot that is its place in the wave
        sr = k[True]["store_rows"]
        with_hist = [i for i, h in zip(k[True]["rm_users"][:, 0].tolist(), nh) if h >= 1]
        assert sorted(sr[:, 0].tolist()) == sorted(with_hist) and sorted(sr[:, 1].tolist()) == list(range(len(with_hist)))
        print(f"  store forwards {k[False]['full'][0]} -> {want[0]} {store}, candidate forwards {k[False]['full'][1]} -> {want[1]}")
        with pytest.raises(ValueError):
            serve.render_users(model, states, pags, registry, pack_ranking=True)
    finally:
        model.close()
