"""GPU: the serving compact top (rsys_serving_compact_top_set) on the whole model -- hd64 dimensions at max_sequence_length 128,
max_rows 4 (tests/_trim_util.config): a plain model, the four-adapter bank and a finetune = 1 model, fp32 and bf16.  Every case runs a
serving call with `compact_top=True` against the same call with the switch off and reads "infer.top" / "infer.top_rows".

Bounds.  fp32: max |on - off| <= 1e-4 max |off| (the project's fp32 bound), and the same against the float64 OracleModel.  bf16: with the
fp32 model's values as the reference, the compact arm's error <= 2 x the dense arm's error measured in the same test (the factor is the
project's allowance for summation order).  K/V-cache slots, the fallbacks, independence and determinism are bit for bit.  Every test prints
its figures.  Observed on an MI355X (also in DESIGN 4ze): fp32 on against off 0.0 - 6.2e-7, against the oracle 3.9e-7 - 1.6e-6 (bound
1e-4); bf16 compact / dense error 0.88 - 1.00 (bound 2); the dense output on demand 0.0 from the switch-off output in both modes.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _adapter_bank_util as ab  # noqa: E402
import _trim_util as tu  # noqa: E402
import test_gpu_rank_cache as trc  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_ROWS = 4
CAP = 256            # rows of the compact buffers at this size: min(tokens, 4 mask_topk max_rows) rounded up to 256
KINDS = ["base", "bank", "ft"]
FT_SLOT = {"retrieval": 0, "ranking": 1}     # the adapter the finetune = 1 model carries, per task (medium 0)
_MODELS = {}


def _make(kind, dtype):
    from oracle import synth
    cfg, V = tu.config()
    if kind != "ft":
        return (cfg, V) + tu.make_model(cfg, kind, dtype, max_rows=MAX_ROWS)
    return cfg, V, None, synth.make_params(cfg, 31, "test"), ab.make_adapters(cfg, 4, 70)


@pytest.fixture(scope="module")
def models():
    """get(kind, dtype, task): (cfg, V, model, P, adapters); the finetune = 1 model carries the adapter of "0.<task>" """
    import recommendersystem_amd as ra

    def get(kind, dtype, task="retrieval"):
        key = (kind, dtype, task if kind == "ft" else "")
        if key not in _MODELS:
            cfg, V, model, P, adapters = _make(kind, dtype)
            if kind == "ft":
                model = ra.RecommenderModel(ab.finetune_config(cfg), dtype=dtype, max_rows=MAX_ROWS)
                model.load_state_dict(dict(P, **adapters[FT_SLOT[task]]))
            _MODELS[key] = (cfg, V, model, P, adapters)
        return _MODELS[key]
    yield get
    for v in _MODELS.values():
        v[2].close()
    _MODELS.clear()


def _top(model):
    return int(model.debug_get("infer.top", 0)[0]), int(model.debug_get("infer.top_rows", 0)[0])


def _flat(res):
    return np.concatenate([np.asarray(v, np.float64).reshape(-1) for r in res for v in r.values()] or [np.zeros(0)])


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if b.size else 0.0


def _check_values(what, dtype, on, off, ref32=None, oracle=None):
    """fp32: on against off and against the oracle; bf16: both arms' error against the fp32 model's values"""
    on, off = _flat(on), _flat(off)
    assert on.shape == off.shape and on.size and np.isfinite(on).all()
    if dtype == "fp32":
        d = _rel(on, off)
        o = _rel(on, oracle) if oracle is not None else float("nan")
        print(f"{what} [fp32] max |on - off| / max |off| {d:.3e}  against the fp64 oracle {o:.3e}")
        assert d <= 1e-4, (what, d)
        assert oracle is None or o <= 1e-4, (what, o)
    else:
        e_on, e_off = _rel(on, ref32), _rel(off, ref32)
        print(f"{what} [bf16] error against the fp32 model: compact {e_on:.3e} dense {e_off:.3e}  ratio {e_on / e_off if e_off else float('nan'):.2f}")
        assert e_on <= 2 * e_off, (what, e_on, e_off)


def _oracle(cfg, P, adapters, kind, users, task, medium):
    return np.concatenate([np.asarray(v, np.float64).reshape(-1) for v in tu.oracle_predict(cfg, P, adapters, "base" if kind == "base" else "bank", users, task, medium)])


HISTS = [1, 31, 32, 33, 127]


# ---------------------------------------------------------------- predict / predict_mixed
@pytest.mark.parametrize("kind", KINDS)
def test_retrieval_one_user_per_row_trimmed(models, kind):
    """histories of 1 / 31 / 32 / 33 and of 127 events, one user per row, trim=True: the query token of every row through attn_sel_kernel"""
    from recommendersystem_amd import serve
    rng = np.random.default_rng(3)
    groups = [[tu.user_with_history(rng, n, []) for n in HISTS[:4]], [tu.user_with_history(rng, 127, [])]]
    vals = {}
    for dtype in ("fp32", "bf16"):
        cfg, V, model, P, adapters = models(kind, dtype)
        assert model.serving_compact_top() is False                         # default off
        for gi, users in enumerate(groups):
            off = serve.predict(model, users, "retrieval", 0, trim=True)
            assert _top(model) == (0, 0)
            on = serve.predict(model, users, "retrieval", 0, trim=True, compact_top=True)
            assert _top(model) == (2, len(users)) and model.serving_compact_top() is False
            vals[(dtype, gi)] = off
            _check_values(f"retrieval rows {kind} group {gi}", dtype, on, off, ref32=_flat(vals[("fp32", gi)]),
                          oracle=_oracle(cfg, P, adapters, kind, users, "retrieval", 0) if dtype == "fp32" else None)


@pytest.mark.parametrize("kind", KINDS)
def test_retrieval_packed_rows(models, kind):
    """pack=True: several users per row (the bank: both media in one row through predict_mixed), each query token a selected query"""
    from recommendersystem_amd import serve
    rng = np.random.default_rng(4)
    users = [tu.user_with_history(rng, n, []) for n in HISTS + [4, 31, 20]]
    media = [i % 2 for i in range(len(users))] if kind == "bank" else [0] * len(users)
    ref32 = None
    for dtype in ("fp32", "bf16"):
        cfg, V, model, P, adapters = models(kind, dtype)
        if kind == "bank":
            call = lambda **kw: serve.predict_mixed(model, list(zip(users, media)), "retrieval", pack=True, **kw)
        else:
            call = lambda **kw: serve.predict(model, users, "retrieval", 0, pack=True, **kw)
        plan = serve.pack_plan([len(serve._history(u, 127)) + 1 for u in users], cfg["max_sequence_length"], MAX_ROWS)
        assert any(len({r for _, r, _ in placed}) < len(placed) for _, placed in plan)      # some row holds several users
        off = call()
        on = call(compact_top=True)
        assert _top(model) == (2, len(plan[-1][1]))                                          # the last forward's users
        oracle = None
        if dtype == "fp32":
            ref32 = _flat(off)
            oracle = np.concatenate([_oracle(cfg, P, adapters, kind, [u], "retrieval", m) for u, m in zip(users, media)])
        _check_values(f"retrieval packed {kind}", dtype, on, off, ref32=ref32, oracle=oracle)


@pytest.mark.parametrize("kind", KINDS)
def test_ranking_on_split_rows(models, kind):
    """predict(..., "ranking"): 4 rows x 20 candidates = 80 action tokens > 4 rows x 4 tiles, 2 x 80 <= 1024 tokens: the compact tail behind
    the dense attention (infer.top 1); 3 candidates per row at trim: the selected-query kernel (infer.top 2)"""
    from recommendersystem_amd import serve
    rng = np.random.default_rng(5)
    V = tu.config()[1]
    requests = {nc: [tu.user_with_history(rng, nh, [int(x) for x in rng.choice(np.arange(1, min(V)), nc, replace=False)]) for nh in (1, 31, 33, 63)]
                for nc in (20, 3)}
    ref32 = {}
    for dtype in ("fp32", "bf16"):
        cfg, V, model, P, adapters = models(kind, dtype, "ranking")
        for nc, trim, mode in ((20, False, 1), (3, True, 2)):
            users = requests[nc]
            off = serve.predict(model, users, "ranking", 0, trim=trim)
            on = serve.predict(model, users, "ranking", 0, trim=trim, compact_top=True)
            assert _top(model) == (mode, 4 * nc)
            assert mode == serve.compact_top_mode(4 * nc, 4, model.batch_row_length, CAP)
            if dtype == "fp32":
                ref32[nc] = _flat(off)
            _check_values(f"ranking split rows {kind} {nc} candidates", dtype, on, off, ref32=ref32[nc],
                          oracle=_oracle(cfg, P, adapters, kind, users, "ranking", 0) if dtype == "fp32" else None)


# ---------------------------------------------------------------- the K/V cache
def _rank_users(rng, V, S, medium):
    """seven histories with 1 / 3 / 33 / S + 5 candidates in turn, a user with an empty history and one without candidates"""
    n_hist, n_cand = [1, 4, 31, 32, 33, 60, 127], [1, 3, 33, S + 5, 3, 33, 1]
    users = [trc.make_user(rng, nh, rng.integers(1, V[medium], size=nc), V) for nh, nc in zip(n_hist, n_cand)]
    users.insert(2, trc.make_user(rng, 0, rng.integers(1, V[medium], size=4), V))
    users.insert(5, trc.make_user(rng, 20, [], V))
    return users


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["base", "bank"])
def test_stopped_store_fills_the_same_slots(models, kind, dtype):
    """rank_cache_store and rank_cache_store_packed with the switch on end at the last layer's K | V copy (infer.top 3); every layer of every
    slot holds the bits the switch-off store wrote"""
    import test_gpu_rank_cache_packed as trp
    cfg, V, model, _, _ = models(kind, dtype)
    L = cfg["num_layers"]
    rng = np.random.default_rng(33)
    users = [trc.make_user(rng, nh, [1], V) for nh in (1, 31, 33, 127)]
    adapter = ab.SLOT_MAP["1.ranking"] if kind == "bank" else None
    model.rank_cache_reserve(16)
    dh, nh = trc._hist_rows(cfg, users, V)
    placed = [(0, 0, 0), (1, 0, 32), (2, 1, 0), (3, 2, 0)]                     # (user, row, first column): users 0 and 1 share a row
    try:
        for on in (False, True):
            model.serving_compact_top(on)
            model.rank_cache_store(dh, nh, [8 * on + u for u in range(4)], adapters=adapter)
            assert _top(model) == ((3, 0) if on else (0, 0))
            d, seg = trp._store_rows(cfg, V, users, [(u, row, c0, 8 * on + 4 + u) for u, row, c0 in placed])
            model.rank_cache_store_packed(d, seg, adapters=adapter, row_len=128)
            assert _top(model) == ((3, 0) if on else (0, 0))
    finally:
        model.serving_compact_top(False)
    for u in range(4):
        for l in range(L):
            assert np.array_equal(model.rank_cache_get(l, u, nh[u]), model.rank_cache_get(l, 8 + u, nh[u])), ("rows", u, l)
            assert np.array_equal(model.rank_cache_get(l, 4 + u, nh[u]), model.rank_cache_get(l, 12 + u, nh[u])), ("packed", u, l)


@pytest.mark.parametrize("pack", [False, True])
@pytest.mark.parametrize("kind", ["base", "bank"])
def test_predict_ranking_full(models, kind, pack):
    """candidate values of predict_ranking_full, plain and packed, with an empty history, a user without candidates and S + 5 candidates"""
    from recommendersystem_amd import serve
    ref32 = None
    for dtype in ("fp32", "bf16"):
        cfg, V, model, P, adapters = models(kind, dtype)
        S = cfg["max_sequence_length"]
        users = _rank_users(np.random.default_rng(21), V, S, 1)
        off = serve.predict_ranking_full(model, users, 1, pack=pack)
        on = serve.predict_ranking_full(model, users, 1, pack=pack, compact_top=True)
        assert [len(r["1.ranking"]) for r in on] == [len(u["ranking_items"]) for u in users]
        assert _top(model)[0] in (1, 2) and model.serving_compact_top() is False
        oracle = None
        if dtype == "fp32":
            ref32 = _flat(off)
            full = [u for u in users if u["items"] and u["ranking_items"]]
            oracle_full = np.concatenate([trc.oracle_full(cfg, P, adapters, kind, dict(u, ranking_items=u["ranking_items"][c0:c0 + S]), 1, V)
                                          for u in full for c0 in range(0, len(u["ranking_items"]), S)])
            got = _flat([r for r, u in zip(on, users) if u["items"] and u["ranking_items"]])
            o = _rel(got, oracle_full)
            print(f"predict_ranking_full pack={pack} {kind} [fp32] compact arm against the fp64 oracle on the reference's row {o:.3e}")
            assert o <= 1e-4, o
        _check_values(f"predict_ranking_full pack={pack} {kind}", dtype, on, off, ref32=ref32)


# ---------------------------------------------------------------- fallbacks
def test_fallbacks_run_dense(models):
    """n_sel > the compact buffers' rows, rsys_infer without a selection and an fp8 model: infer.top 0 and the switch-off bits"""
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import serve
    cfg, V, model, _, _ = models("base", "fp32")
    S = cfg["max_sequence_length"]
    rng = np.random.default_rng(6)
    users = [tu.user_with_history(rng, n, []) for n in (5, 40, 90, 127)]
    d = serve.build_batch(users, "retrieval", 0, V[0], *serve._request_lengths(model, "retrieval", None, None))
    index = list(range(0, 2 * (CAP + 44), 2))                                   # 300 tokens: 2 x 300 <= 1024, but more than the buffers hold
    assert len(index) > CAP and 2 * len(index) <= MAX_ROWS * 2 * S
    try:
        res = {}
        for on in (False, True):
            model.serving_compact_top(on)
            res[on] = [model.inference_select(d, "retrieval", index).copy()]
            assert _top(model) == (0, 0)
            res[on].append(np.asarray(model.inference_forward(d, "retrieval")).copy())
            assert _top(model) == (0, 0)
            res[on].append(model.inference_select(d, "ranking", index[:CAP]).copy())       # exactly the buffers' rows: compact
            assert _top(model) == ((1, CAP) if on else (0, 0))
    finally:
        model.serving_compact_top(False)
    assert np.array_equal(res[False][0], res[True][0]) and np.array_equal(res[False][1], res[True][1])
    assert _rel(res[True][2].astype(np.float64), res[False][2].astype(np.float64)) <= 1e-4
    cfg8 = synth.make_config("f8t", mask_rate=0.2, mask_topk=16)
    m8 = ra.RecommenderModel(cfg8, device=0, dtype="fp8", max_rows=2)
    try:
        m8.load_state_dict(synth.make_params(cfg8, 23, "test"))
        d8 = synth.make_batch(cfg8, 2, 24)
        a = m8.inference_select(d8, "retrieval", [1, 3, 5]).copy()
        m8.serving_compact_top(True)
        b = m8.inference_select(d8, "retrieval", [1, 3, 5]).copy()
        assert _top(m8) == (0, 0) and np.array_equal(a, b)
    finally:
        m8.close()


# ---------------------------------------------------------------- the dense output on demand
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_trunk_output_after_a_compact_pass_and_a_stopped_store(models, dtype):
    """rsys_trunk_output_get after infer.top 2, 1 and 3 is the switch-off output: token order was kept and the rest runs as the dense pass
    would have, on the same GEMM routes -- bit for bit in fp32; bf16: its error against the fp32 model's output <= 2 x the switch-off
    output's"""
    from recommendersystem_amd import serve
    cfg, V, model, _, _ = models("bank", dtype)
    f32 = models("bank", "fp32")[2]
    S = cfg["max_sequence_length"]
    rng = np.random.default_rng(7)
    users = [tu.user_with_history(rng, n, [int(x) for x in rng.choice(np.arange(1, min(V)), 20, replace=False)]) for n in (5, 31, 40, 63)]
    ret_len, rank_len = (serve._request_lengths(model, t, None, None) for t in ("retrieval", "ranking"))
    d_ret = serve.build_batch(users, "retrieval", 0, V[0], *ret_len)
    tok, _ = serve._selected_tokens(users, "retrieval", S, ret_len[0])
    d_rank = serve.build_batch(users, "ranking", 0, V[0], *rank_len)
    rtok, _ = serve._selected_tokens(users, "ranking", S, rank_len[0])
    hu = [trc.make_user(rng, nh, [1], V) for nh in (1, 31, 33, 127)]
    dh, nh = trc._hist_rows(cfg, hu, V)
    model.rank_cache_reserve(4)
    f32.rank_cache_reserve(4)
    passes = [("attn_sel", 2, lambda m: m.inference_select(d_ret, "retrieval", tok, adapters=[0] * 4)),
              ("gathered", 1, lambda m: m.inference_select(d_rank, "ranking", rtok, adapters=[1] * 4)),
              ("stopped store", 3, lambda m: m.rank_cache_store(dh, nh, [0, 1, 2, 3], adapters=3))]
    try:
        for what, mode, run in passes:
            model.serving_compact_top(False)
            run(model)
            want = model.trunk_output(4).copy()
            model.serving_compact_top(True)
            run(model)
            assert _top(model)[0] == mode
            got = model.trunk_output(4).copy()
            again = model.trunk_output(4).copy()                                # (materialised once; a second read finds it)
            d = _rel(got.astype(np.float64), want.astype(np.float64))
            print(f"trunk output after {what} [{dtype}]: max |on - off| / max |off| {d:.3e}")
            assert np.array_equal(got, again)
            if dtype == "fp32":
                assert np.array_equal(got, want), (what, d)
            else:
                run(f32)
                ref = f32.trunk_output(4).astype(np.float64)
                e_on, e_off = _rel(got.astype(np.float64), ref), _rel(want.astype(np.float64), ref)
                print(f"  error against the fp32 model's output: after the compact pass {e_on:.3e}, switch off {e_off:.3e}")
                assert e_on <= 2 * e_off, (what, e_on, e_off)
    finally:
        model.serving_compact_top(False)


# ---------------------------------------------------------------- independence and determinism
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_users_of_one_packed_forward_do_not_see_each_other(models, dtype):
    """A, B and C share a packed compact forward, A and B a row: replacing B's events or B's adapter leaves A's and C's values bit-identical"""
    from recommendersystem_amd import serve
    cfg, V, model, _, _ = models("bank", dtype)
    rng = np.random.default_rng(8)
    A, B, C, B2 = (tu.user_with_history(rng, n, []) for n in (33, 4, 100, 9))

    def run(b, b_medium):
        res = serve.predict_mixed(model, [(A, 0), (b, b_medium), (C, 1)], "retrieval", pack=True, compact_top=True)
        assert _top(model) == (2, 3)
        return [np.asarray(list(r.values())[0], np.float32) for r in res]

    a0, b0, c0 = run(B, 0)
    for b, m in ((B2, 0), (B, 1)):
        a1, b1, c1 = run(b, m)
        assert np.array_equal(a0, a1) and np.array_equal(c0, c1) and not np.array_equal(b0, b1)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_compact_inference_between_training_steps_changes_nothing(dtype):
    """deterministic mode: step -> compact inference calls -> step gives the step -> step results bit for bit"""
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import serve
    cfg = synth.make_config("hd64", mask_rate=0.2, deterministic=True)
    V = (cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"])
    P = synth.make_params(cfg, 3, "test")
    rows = 4
    batches = [synth.make_batch(cfg, rows, 40 + i) for i in range(2)]
    masks = [synth.make_masks(cfg, rows, 50 + i) for i in range(2)]
    names = synth.trainable_names(cfg)
    rng = np.random.default_rng(2)
    users = [tu.user_with_history(rng, 5, [3, 4, 5]), tu.user_with_history(rng, 20, [6, 7])]
    full = [trc.make_user(rng, 30, [1, 2, 3], V), trc.make_user(rng, 9, [4], V)]

    def run(with_inference):
        model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
        model.load_state_dict(P)
        opt = ra.create_optimizer(model, dict(cfg, learning_rate=1e-2))
        model.set_loss_weights([0.05, 0.2, 0.3, 0.25], 1)
        out = []
        for i, (d, mk) in enumerate(zip(batches, masks)):
            if i == 1 and with_inference:
                serve.predict(model, users, "retrieval", 0, trim=True, compact_top=True)
                assert _top(model)[0] == 2
                serve.predict(model, users, "ranking", 0, compact_top=True)
                assert _top(model)[0] in (1, 2)
                serve.predict_ranking_full(model, full, 1, compact_top=True)
                model.serving_compact_top(True)                                  # (a training pass does not read the switch)
            out.append(np.array(model(d, False, masks=mk), np.float32))
            out += [model.grad(n).copy() for n in names]
            opt.step(clip_max_norm=1.0)
        out += [model.get_parameter(n).copy() for n in names]
        model.close()
        return out

    a, b = run(False), run(True)
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- the render pipeline
# Request seeds of test_gpu_render_request._request, chosen per model kind from a scan of seeds 40 .. 139 with the switch off (fp32): the
# smallest gap between adjacent final scores at or above a page's last rank, as a fraction of the largest |score|, is 3.31e-4 (base, seed
# 59) and 2.87e-4 (bank, seed 74); the default seed 40 gives 1.6e-5 for both, and no seed of the scan reaches 2e-4 for both kinds.  The
# test recomputes the gap from the switch-off arm and asserts it.
RENDER_SEED = {"base": 59, "bank": 74}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["base", "bank"])
def test_render_users_full_history_packed(kind, dtype):
    """render_users(full_history=True, pack=True, pack_ranking=True, compact_top=True) against compact_top=False on the 5 states / 9 users of
    tests/test_gpu_rank_cache_packed.py: totals equal, r_masked within the value bounds, and in fp32 every page's ids equal -- the request
    (seed RENDER_SEED[kind]) is checked to have no two adjacent final scores at or above a page's last rank closer than twice the fp32 bound
    (2e-4 of the largest |score|), so a difference inside the bound cannot swap two of them.  The forward counters are
    serve.render_full_forwards' with the switch on as with it off, and "forward_top" reports every forward: every store stopped (3), every
    other forward what serve.compact_top_mode says for the rows it reports."""
    import test_gpu_render_full as rf
    import test_gpu_render_request as rq
    from recommendersystem_amd import serve
    cfg, V = tu.config()
    model, _, _ = tu.make_model(cfg, kind, dtype, max_rows=MAX_ROWS)
    try:
        S, RM = cfg["max_sequence_length"], model.max_rows
        rq._tables(model, V)
        states, pags, registry = rq._request(seed=RENDER_SEED[kind])
        states[0]["users"][0]["user"]["items"] = []                            # a user with an empty history
        assert sum(len(st["users"]) for st in states) == 9 and len(states) == 5
        model.rank_cache_reserve(8)
        model.render_keep(True)
        res, k, fr, ft = {}, {}, {}, {}
        for on in (False, True):
            res[on] = serve.render_users(model, states, pags, registry, full_history=True, pack=True, pack_ranking=True, compact_top=on)
            k[on] = rf._kept(model, cfg, states)
            fr[on] = model.render_kept("forward_rows").reshape(-1, 3).copy()
            ft[on] = model.render_kept("forward_top").reshape(-1, 2).copy()
            assert model.serving_compact_top() is False
        assert [t for _, t in res[False]] == [t for _, t in res[True]]
        a, b = k[True]["r_masked"].astype(np.float64), k[False]["r_masked"].astype(np.float64)
        assert a.shape == b.shape and a.size
        d = _rel(a, b)
        print(f"render {kind} [{dtype}]: r_masked max |on - off| / max |off| {d:.3e}")
        if dtype == "fp32":
            assert d <= 1e-4, d
            active, _ = rf._windows(k[False], states, pags, res[False])
            gap = np.inf
            for g, (_, _, c0, n, sidx, eidx) in ((g, tuple(int(x) for x in r)) for g, r in active.items()):
                r = np.sort(k[False]["r"][c0:c0 + n].astype(np.float64))[::-1][:eidx + 1]
                if r.size > 1:
                    gap = min(gap, float(np.min(-np.diff(r)) / np.abs(k[False]["r"]).max()))
            print(f"render {kind} [fp32] seed {RENDER_SEED[kind]}: smallest gap between adjacent scores at or above a page's last rank {gap:.3e} of max |score|")
            assert gap >= 2e-4, gap
            assert len(res[False]) == len(res[True]) == 5
            for (pa, _), (pb, _) in zip(res[False], res[True]):                 # every page, every position
                assert np.array_equal(pa, pb)
        else:
            f32, _, _ = tu.make_model(cfg, kind, "fp32", max_rows=MAX_ROWS)
            try:
                rq._tables(f32, V)
                f32.rank_cache_reserve(8)
                f32.render_keep(True)
                serve.render_users(f32, states, pags, registry, full_history=True, pack=True, pack_ranking=True)
                ref = f32.render_kept("r_masked").astype(np.float64)
            finally:
                f32.close()
            assert ref.shape == a.shape
            e_on, e_off = _rel(a, ref), _rel(b, ref)
            print(f"render {kind} [bf16] r_masked error against the fp32 model: compact {e_on:.3e} dense {e_off:.3e}")
            assert e_on <= 2 * e_off, (e_on, e_off)
        _, cand_of = rf._windows(k[True], states, pags, res[True])
        _, _, nh, nc = rf._plan_inputs(k[True], cfg, states, cand_of)
        want = serve.render_full_forwards(nh, nc, S, RM, pack_store=True, slots=8)
        assert k[True]["full"].tolist() == k[False]["full"].tolist() == list(want)
        assert np.array_equal(fr[True], fr[False]) and len(ft[True]) == len(fr[True]) == len(ft[False])
        assert not ft[False].any()
        seen = set()
        for (stage, rows, row_len), (mode, n) in zip(fr[True].tolist(), ft[True].tolist()):
            seen.add(mode)
            if stage == 1:
                assert (mode, n) == (3, 0)
            elif mode:
                assert mode == serve.compact_top_mode(n, rows, row_len, CAP, "candidates" if stage == 2 else "select"), (stage, rows, row_len, mode, n)
            else:
                assert stage != 0                                               # a retrieval forward reports one token per user: always compact
        print(f"  forward_rows {fr[True].tolist()} forward_top {ft[True].tolist()}")
        assert 3 in seen and 2 in seen
    finally:
        model.close()
