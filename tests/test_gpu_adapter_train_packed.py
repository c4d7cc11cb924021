"""GPU: training the finetune adapters on packed rows (rsys_adapter_forward_backward_packed, train.pack_adapter_rows): several
users per batch row, each in a segment of whole 64-token tiles that names its slot and task.

Set-up: hd64 dimensions at max_sequence_length 128, mask_topk 16, at most 8 rows.  Eight users cut from oracle.synth rows -- the first n
columns of row u as ONE user, n = 4, 5, 31, 32, 33, 60, 64, 128, zeros behind -- each thinned to at most 4 targets per task: the finetune
rows of DESIGN 4y's tests with a live prefix.  `serve.pack_plan` puts them into 4 rows.  Slot s runs task s; user 4 runs the base model.
The host asserts, before any GPU run, that every slot has a target of its task and that the selection (mask_topk x rows per task) holds
every target in the packed (4 rows) and the unpacked (8 rows) batch and in each slot's oracle batch."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _adapter_bank_util as ab  # noqa: E402
from test_gpu_adapter_train import FP32_TOL, METRICS, _errors, _task_cfg, relerr  # noqa: E402

pytestmark = pytest.mark.gpu

S, ROWS_MAX, KEEP, SEED = 128, 8, 4, 21
LIVE = [4, 5, 31, 32, 33, 60, 64, 128]
SLOTS = [0, 1, 2, 3, -1, 2, 0, 1]          # slot s runs task s: two users each for slots 0, 1, 2, one for slot 3, one base-model user
USERS = len(LIVE)


@pytest.fixture
def dense_top(monkeypatch):
    """RSYS_SPARSE_TOP=0 for the models the test creates; the environment and the parsed switches are restored afterwards"""
    from recommendersystem_amd._lib import lib
    monkeypatch.setenv("RSYS_SPARSE_TOP", "0")
    lib().rsys_switches_reload()
    yield
    monkeypatch.undo()
    lib().rsys_switches_reload()


def _cut(cfg, d, live, keep=KEEP):
    """row u of `d` as one finetune row: its first live[u] columns as ONE user (userid 100 + u), at most `keep` targets per task, zeros
    behind the prefix"""
    out = {k: np.array(np.asarray(v).reshape(-1, S)) for k, v in d.items()}
    for u, n in enumerate(live):
        for k, v in out.items():
            v[u, n:] = 0
        out["userid"][u, :n] = 100 + u
        for m in (0, 1):
            for x in METRICS:
                w = out[f"{m}.{x}.weight"]
                on = np.flatnonzero(w[u] > 0)
                w[u, on[keep:]] = 0
    return {k: v[:len(live)] for k, v in out.items()}


def _subs(rows, users=None, slots=SLOTS):
    """the users as sub-batches in user order: what the loaders hand to the packers (one sub-batch per user keeps the order free)"""
    return [(slots[u], slots[u], {k: v[u].copy() for k, v in rows.items()}) for u in (range(len(slots)) if users is None else users)]


_SETUP = {}


def _setup(seed_shift=0):
    if seed_shift not in _SETUP:
        from oracle import synth
        from recommendersystem_amd.train import pack_adapter_batch, pack_adapter_rows
        cfg = synth.make_config("hd64", mask_rate=0.2, mask_topk=16, max_sequence_length=S)
        K = cfg["mask_topk"]
        P = synth.make_params(cfg, SEED, "test")
        rows = _cut(cfg, synth.make_batch(cfg, USERS, SEED + 1 + seed_shift), LIVE)
        adapters = ab.make_adapters(cfg, 4, SEED + 50)
        packed, segs = pack_adapter_rows(_subs(rows), S, ROWS_MAX, K)
        flat, rs, rt = pack_adapter_batch(_subs(rows), S)
        assert rs.tolist() == SLOTS and packed["userid"].size == 4 * S and segs[:, 3].tolist() == SLOTS
        for s in range(4):
            mine = [u for u in range(USERS) if SLOTS[u] == s]
            own = rows[f"{s >> 1}.{METRICS[s & 1]}.weight"][mine]
            assert (own > 0).sum() >= 1, ("no target", s)
            for m in (0, 1):
                for x in METRICS:        # per task: the packed pass's selection, the unpacked pass's, the oracle run on the slot's own rows
                    n_all = int((rows[f"{m}.{x}.weight"] > 0).sum())
                    assert n_all <= K * 4 and n_all <= K * USERS, (m, x, n_all)
                    assert int((rows[f"{m}.{x}.weight"][mine] > 0).sum()) <= K * len(mine), (s, m, x)
        _SETUP[seed_shift] = (cfg, P, rows, adapters, packed, segs, flat)
    return _SETUP[seed_shift]


_ORACLE = {}


def _oracle(s, users=None, tag=None):
    """losses, weight sum and LoRA gradients of adapter s in float64 on its users, each in a row of its own"""
    key = (s, tag)
    if key not in _ORACLE:
        from oracle import model_np
        cfg, P, rows, adapters = _setup()[:4]
        mine = [u for u in range(USERS) if SLOTS[u] == s] if users is None else users
        ft = _task_cfg(cfg, s)
        sub = {k: np.ascontiguousarray(v[mine].reshape(-1)) for k, v in rows.items()}
        dm = model_np.mask_tokens(ft, model_np.reshape_batch(ft, sub))
        tw = [1.0 if i == s else 0.0 for i in range(4)]
        losses, G = model_np.OracleModel(ft, dict(P, **adapters[s]), np.float64).forward(dm, False, True, tw)
        wsum = float(dm[f"{s >> 1}.{METRICS[s & 1]}.weight"].sum())
        _ORACLE[key] = (float(losses[s]), wsum, {k: G[k] for k in adapters[s]})
    return _ORACLE[key]


def _bank(dtype, dropout=0.0, adapters=None, n=4):
    import recommendersystem_amd as ra
    cfg, P, rows, ads = _setup()[:4]
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=ROWS_MAX)
    model.load_state_dict(P)
    for s, ad in enumerate((ads if adapters is None else adapters)[:n]):
        model.load_adapter(s, ad)
    model.enable_adapter_training(dropout)
    return model


def _grads(bank, n=4):
    return {(s, k): v for s in range(n) for k, v in bank.adapter_grad(s).items()}


def _packed_pass(bank, packed, segs, micro=1, **kw):
    bank.upload(packed)
    bank.zero_adapter_grads()
    for _ in range(micro):
        losses = bank.forward_backward_adapters_packed(None, segs, grad_scale=1.0 / micro, **kw)
    return losses, list(bank.last_weight_sums), _grads(bank)


def _flat_pass(bank, flat, micro=1, **kw):
    bank.upload(flat)
    bank.zero_adapter_grads()
    for _ in range(micro):
        losses = bank.forward_backward_adapters(None, SLOTS, SLOTS, grad_scale=1.0 / micro, **kw)
    return losses, list(bank.last_weight_sums), _grads(bank)


def _slot_errors(res, refs):
    losses, wsums, g = res
    return np.array([_errors((losses[s], wsums[s], {k: g[(s, k)] for k in refs[s][2]}), refs[s]) for s in range(4)])


# ============================================================================================ 1, 4a: parity against the oracle
@pytest.mark.parametrize("micro", [1, 2], ids=["one pass", "two micro-steps at 1/2"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_parity_against_the_oracle(dtype, micro):
    """fp32: every quantity < 1e-4 (gradients relative to each tensor's maximum).  bf16: the packed pass's error <= 1.5 x the unpacked joint
    pass's error against the same oracle, per quantity, worst slot each (test_gpu_adapter_train.py's rule)."""
    cfg, P, rows, adapters, packed, segs, flat = _setup()
    refs = [_oracle(s) for s in range(4)]
    assert all(r[0] > 0 and r[1] > 0 and all(np.abs(v).max() > 0 for v in r[2].values()) for r in refs)
    bank = _bank(dtype)
    ep = _slot_errors(_packed_pass(bank, packed, segs, micro), refs)
    eu = _slot_errors(_flat_pass(bank, flat, micro), refs)
    bank.close()
    print(f"packed adapter training {dtype} micro {micro}: errors per slot (loss, weight sum, gradient) packed {ep.tolist()}, unpacked {eu.tolist()}")
    if dtype == "fp32":
        assert ep.max() < FP32_TOL, ep
    else:
        for q in range(3):
            assert ep[:, q].max() <= 1.5 * eu[:, q].max(), (q, ep[:, q], eu[:, q])


# ============================================================================================ 2: packed against unpacked, both dense
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_packed_against_unpacked_dense_top(dtype, dense_top):
    """The unpacked pass with the last layer dense (RSYS_SPARSE_TOP=0), as the packed pass always runs it: the same users, the same
    arithmetic per token, the same order of every sum a slot's gradient consists of.  Measured on an MI355X: see the
    assertion."""
    cfg, P, rows, adapters, packed, segs, flat = _setup()
    bank = _bank(dtype)
    lp, wp, gp = _packed_pass(bank, packed, segs, step=3)
    lu, wu, gu = _flat_pass(bank, flat, step=3)
    ev_p = (bank.upload(packed), bank.forward_backward_adapters_packed(None, segs, evaluate=True), list(bank.last_weight_sums))[1:]
    ev_u = (bank.upload(flat), bank.forward_backward_adapters(None, SLOTS, SLOTS, evaluate=True), list(bank.last_weight_sums))[1:]
    bank.close()
    worst = max(relerr(gp[k], gu[k]) for k in gp)
    nbits = sum(int((gp[k].view(np.uint32) != gu[k].view(np.uint32)).sum()) for k in gp)
    dl = max(abs(a - b) / abs(b) for a, b in zip(lp, lu))
    flat_l = lambda v: [x for e in v for x in (e if isinstance(e, list) else [e])]
    dev = max(abs(a - b) / max(abs(b), 1e-30) for a, b in zip(flat_l(ev_p[0]), flat_l(ev_u[0])))
    print(f"packed vs unpacked, dense top, {dtype}: worst gradient difference {worst:.3e} ({nbits} values differ), worst loss difference {dl:.3e}, "
          f"weight sums {wp} / {wu}, evaluation moments differ by {dev:.3e}")
    assert wp == wu and ev_p[1] == ev_u[1]
    assert nbits == 0 and lp == lu and ev_p[0] == ev_u[0]


# ============================================================================================ 3, 4b: isolation, repeats
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_isolation_and_equal_bits(dtype):
    from recommendersystem_amd.train import pack_adapter_rows
    cfg, P, rows, adapters, packed, segs, flat = _setup()
    other = _setup(seed_shift=7)[2]
    bank = _bank(dtype, adapters=adapters + [adapters[0]], n=5)          # slot 4: complete, never named
    l1, w1, g1 = _packed_pass(bank, packed, segs, step=3)
    l2, w2, g2 = _packed_pass(bank, packed, segs, step=3)
    assert l1 == l2 and w1 == w2 and all(np.array_equal(g1[k], g2[k]) for k in g1)          # a repeated call: equal bits
    assert all(g1[(s, k)].any() for s in range(4) for k in adapters[s])
    assert all(not g.any() for g in bank.adapter_grad(4).values())
    # user 5 (slot 2) gets other events of the same length: slots 0, 1, 3 keep their bits
    swapped = {k: v.copy() for k, v in rows.items()}
    for k in swapped:
        swapped[k][5] = other[k][5]
    swapped["userid"][5, :LIVE[5]] = 105
    p2, s2 = pack_adapter_rows(_subs(swapped), S, ROWS_MAX, cfg["mask_topk"])
    assert np.array_equal(s2, segs)
    _, _, g3 = _packed_pass(bank, p2, s2, step=3)
    # user 5 moves to the base model: the same
    to_base = [(-1 if u == 5 else s) for u, s in enumerate(SLOTS)]
    p4, s4 = pack_adapter_rows(_subs(rows, slots=to_base), S, ROWS_MAX, cfg["mask_topk"])
    _, _, g4 = _packed_pass(bank, p4, s4, step=3)
    for s in (0, 1, 3):
        for k in adapters[s]:
            assert np.array_equal(g1[(s, k)], g3[(s, k)]) and np.array_equal(g1[(s, k)], g4[(s, k)]), (s, k)
    assert any(not np.array_equal(g1[(2, k)], g3[(2, k)]) for k in adapters[2])
    assert any(not np.array_equal(g1[(2, k)], g4[(2, k)]) for k in adapters[2])
    # another plan: one user per row, each at another tile offset (8 rows instead of 4), descriptors in the same order
    alt = [32, 64, 96, 64, 0, 32, 64, 0]
    wide = {k: np.zeros((USERS, S), v.dtype) for k, v in packed.items()}
    s5 = segs.copy()
    for u, (row, c0, n, _, _) in enumerate(segs):
        for k, v in packed.items():
            wide[k][u, alt[u]:alt[u] + n] = v.reshape(-1, S)[row, c0:c0 + n]
        s5[u, :2] = (u, alt[u])
    l5, w5, g5 = _packed_pass(bank, {k: v.reshape(-1) for k, v in wide.items()}, s5, step=3)
    bank.close()
    nbits = sum(int((g1[k].view(np.uint32) != g5[k].view(np.uint32)).sum()) for k in g1)
    worst = max(relerr(g5[k], g1[k]) for k in g1)
    print(f"packed, {dtype}: the plan of 8 rows against the plan of 4: {nbits} gradient values differ (worst {worst:.3e}), losses {l5} / {l1}")
    assert w5 == w1 and nbits == 0


# ============================================================================================ 4c: dropout, a repeated user
def test_dropout_fresh_masks_same_key_same_bits_evaluation_without():
    cfg, P, rows, adapters, packed, segs, flat = _setup()
    bank = _bank("fp32", dropout=0.5)
    bank.upload(packed)
    fb = lambda step, ev=False: bank.forward_backward_adapters_packed(None, segs, evaluate=ev, step=step)
    a = fb(1); ga = _grads(bank); bank.zero_adapter_grads()
    b = fb(2); bank.zero_adapter_grads()
    c = fb(1); gc = _grads(bank); bank.zero_adapter_grads()
    assert a == c and all(np.array_equal(ga[k], gc[k]) for k in ga)
    assert all(abs(a[i] - b[i]) > 1e-6 * abs(a[i]) for i in range(4)), (a, b)
    ev = fb(1, True)
    bank.enable_adapter_training(0.0)
    assert ev == fb(1, True) and ev == fb(9, True)
    bank.close()


@pytest.mark.parametrize("dtype", ["fp32"])
def test_a_repeated_user_in_one_row_counts_twice(dtype):
    """the loader pads batches with random repeats: the same events twice in one row, under distinct segment ids, give twice that user's
    contribution -- the oracle on the user's row twice (two rows), within the parity bound"""
    from oracle import model_np
    from recommendersystem_amd.train import pack_adapter_rows
    cfg, P, rows, adapters = _setup()[:4]
    users = [2, 2, 3]                                                    # user 2 (31 events, slot 2) twice, user 3 (slot 3)
    subs = [(SLOTS[u], SLOTS[u], {k: v[u].copy() for k, v in rows.items()}) for u in users]
    packed, segs = pack_adapter_rows(subs, S, ROWS_MAX, cfg["mask_topk"])
    uid = packed["userid"].reshape(-1, S)
    assert uid.shape[0] == 1 and segs[:, 0].tolist() == [0, 0, 0] and len(set(uid[0, c0] for _, c0, _, _, _ in segs)) == 3
    bank = _bank(dtype)
    res = _packed_pass(bank, packed, segs)
    bank.close()
    ref = _oracle(2, users=[2, 2], tag="twice")
    once = _oracle(2, users=[2], tag="once")
    assert abs(ref[1] - 2 * once[1]) < 1e-9 * ref[1]
    e = _errors((res[0][2], res[1][2], {k: res[2][(2, k)] for k in ref[2]}), ref)
    print(f"a user twice in one row, {dtype}: errors (loss, weight sum, gradient) {e}")
    assert max(e) < FP32_TOL, e


# ============================================================================================ 5: three joint optimizer steps
OPT_SCALE, OPT_LR = [1.0, 1.0, 0.005, 0.01], 1e-4


@pytest.mark.parametrize("dtype,tol", [("fp32", 3e-4), ("bf16", 8e-2)])
def test_three_joint_optimizer_steps_on_packed_batches(dtype, tol):
    """test_gpu_adapter_train.py's test_three_joint_optimizer_steps on packed batches: norms within 3e-4 (fp32) / 8e-2 (bf16) of
    oracle.train_np's, parameters within 3e-4 in fp32; in bf16 the packed run's parameter error <= 1.5 x the unpacked joint run's"""
    from oracle import model_np, train_np
    from recommendersystem_amd.optim import AdapterAdamW
    cfg, P, rows, adapters, packed, segs, flat = _setup()
    scaled = [{k: v * np.float32(OPT_SCALE[s]) for k, v in adapters[s].items()} for s in range(4)]
    ref_P, ref_norms = [], []
    for s in range(4):
        mine = [u for u in range(USERS) if SLOTS[u] == s]
        ft = _task_cfg(cfg, s)
        sub = {k: np.ascontiguousarray(v[mine].reshape(-1)) for k, v in rows.items()}
        dm = model_np.mask_tokens(ft, model_np.reshape_batch(ft, sub))
        Ps = {k: np.asarray(v, np.float64) for k, v in dict(P, **scaled[s]).items()}
        names = list(scaled[s])
        opt = train_np.AdamW(Ps, names, OPT_LR)
        norms = []
        for _ in range(3):
            _, G = model_np.OracleModel(ft, Ps, np.float64).forward(dm, False, True, [1.0 if i == s else 0.0 for i in range(4)])
            G, norm = train_np.clip_grad_norm({k: G[k] for k in names}, 1.0)
            Ps = opt.step(dict(Ps), G)
            norms.append(norm)
        ref_P.append(Ps); ref_norms.append(norms)
    print(f"packed adapter optimizer {dtype}: oracle norms per slot and step {ref_norms}")

    def three(pack):
        bank = _bank(dtype, adapters=scaled)
        opt = AdapterAdamW(bank, lr=OPT_LR, slots=range(4))
        bank.upload(packed if pack else flat)
        for step in range(3):
            if pack:
                bank.forward_backward_adapters_packed(None, segs)
            else:
                bank.forward_backward_adapters(None, SLOTS, SLOTS)
            norms = opt.step({s: 1.0 for s in range(4)}, clip_max_norm=1.0)
            if pack:
                for s in range(4):
                    assert abs(norms[s] - ref_norms[s][step]) < tol * ref_norms[s][step], (step, s, norms[s], ref_norms[s][step])
        worst = max(relerr(v, ref_P[s][k]) for s in range(4) for k, v in bank.adapter_state_dict(s).items())
        assert [opt.state_dict()[s]["step"] for s in range(4)] == [3] * 4
        bank.close()
        return worst

    worst = three(True)
    if dtype == "fp32":
        print(f"packed adapter optimizer fp32: worst parameter error after three steps {worst:.3e}")
        assert worst < tol, worst
        return
    worst_u = three(False)
    print(f"packed adapter optimizer bf16: worst parameter error after three steps: packed {worst:.3e}, unpacked {worst_u:.3e}")
    assert worst <= 1.5 * worst_u, (worst, worst_u)


# ============================================================================================ 6: the model is left untouched; refusals
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_packed_training_leaves_the_model_untouched(dtype):
    """state_dict, item table, an rsys_infer_select result and the losses and gradients of a following deterministic ordinary step are
    bit-equal to a model that never had a bank (the packed pass runs the last layer dense on a model whose ordinary step runs it compact)"""
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd.optim import AdapterAdamW
    cfg, P, rows, adapters, packed, segs, flat = _setup()
    d = synth.make_batch(cfg, ROWS_MAX, 77)
    wm, rm = synth.make_masks(cfg, ROWS_MAX, 7)
    idx = np.arange(0, ROWS_MAX * 2 * S, 5, dtype=np.int32)
    di = dict(d, rope_input_pos=np.tile(np.arange(S, dtype=np.int32), ROWS_MAX))
    grads = ["transformers.layers.0.attn.q_proj.weight", "transformers.layers.1.mlp.w2.weight", "item_embedding.projection_layer.weight",
             "item_embedding.matchedid_embedding.embedding.weight", "rating_head.0.weight", "rating_head.2.bias", "norm.scale",
             "transformers.layers.0.sa_norm.scale"]

    def observe(with_bank):
        m = ra.RecommenderModel(dict(cfg, forward="train"), dtype=dtype, max_rows=ROWS_MAX)
        m.set_deterministic(True)
        m.load_state_dict(P)
        names = [n for n, _, _ in m.named_parameters()]
        if with_bank:
            for s, ad in enumerate(adapters):
                m.load_adapter(s, ad)
            m.enable_adapter_training(0.1)
            opt = AdapterAdamW(m, lr=1e-2, slots=range(4))
            for step in range(2):
                m.forward_backward_adapters_packed(packed, segs)
                m.forward_backward_adapters_packed(packed, segs, evaluate=True)
                opt.step({s: 1.0 for s in range(4)}, clip_max_norm=1.0)
        sd = m.state_dict()
        table = m.item_embeddings()
        sel = m.inference_select(di, "ranking", idx)
        m.set_loss_weights([0.05, 0.2, 0.3, 0.25])
        losses = m({k: v for k, v in d.items()}, False, masks=(wm, rm))
        g = {k: m.grad(k) for k in grads if k in names}
        m.close()
        return sd, table, sel, losses, g

    a, b = observe(False), observe(True)
    assert sorted(a[0]) == sorted(b[0]) and all(np.array_equal(a[0][k], b[0][k]) for k in a[0])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[3] == b[3], (a[3], b[3])
    assert len(a[4]) >= 5 and all(np.array_equal(a[4][k], b[4][k]) for k in a[4])


def test_argument_errors_leave_everything_unwritten():
    import recommendersystem_amd as ra
    from recommendersystem_amd._lib import lib
    cfg, P, rows, adapters, packed, segs, flat = _setup()
    Lb, ARG, STATE = lib(), -1, -3
    call = lambda h, sg, n=None: Lb.rsys_adapter_forward_backward_packed(h, 0, None if sg is None else sg.ctypes.data,
                                                                         (0 if sg is None else len(sg)) if n is None else n, 1.0, 1, 0)
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=ROWS_MAX)
    model.load_state_dict(P)
    for s in range(3):
        model.load_adapter(s, adapters[s])
    h = model._h
    model.upload(packed)
    assert call(h, segs) == ARG                                                    # training not enabled
    model.enable_adapter_training(0.0)
    assert call(h, segs) == ARG                                                    # slot 3 is not loaded: incomplete
    model.load_adapter(3, adapters[3])
    model.forward_backward_adapters_packed(None, segs)
    keep_l, keep_w = model.losses(), list(model.last_weight_sums)
    keep_g = _grads(model)

    def unchanged():
        assert model.losses() == keep_l and list(model.last_weight_sums) == keep_w
        assert all(np.array_equal(v, model.adapter_grad(s, k)) for (s, k), v in keep_g.items())

    def edit(i, **kw):
        t = segs.copy()
        for name, v in kw.items():
            t[i, ("row", "c0", "cols", "slot", "task").index(name)] = v
        return t

    u128 = int(np.flatnonzero(segs[:, 2] == 128)[0]); u4 = int(np.flatnonzero(segs[:, 2] == 4)[0]); u5 = int(np.flatnonzero(segs[:, 2] == 5)[0])
    bad = [edit(u4, c0=16), edit(u4, c0=int(segs[u4, 1]) + 8),                     # first_column % 32 != 0
           edit(u128, cols=129), edit(u4, cols=0), edit(u4, c0=128), edit(u4, row=4), edit(u4, row=-1),       # outside its row / the batch
           edit(u4, c0=int(segs[u5, 1])),                                          # two segments share a tile
           edit(u4, slot=8), edit(u4, slot=5), edit(u4, task=4),                   # out of range, an empty slot
           edit(u4, slot=-1), edit(u4, task=-1),                                   # a slot without a task and the reverse
           edit(u4, task=3)]                                                       # task 3 named by slot 0 and slot 3
    for t in bad:
        assert call(h, t) == ARG, t.tolist()
        unchanged()
    assert call(h, None, 8) == ARG and call(h, segs, 0) == ARG and call(h, segs, -1) == ARG
    many = np.concatenate([segs] * 3)[:17]                                         # 17 > 4 rows x ceil(128 / 32) = 16
    assert call(h, many) == ARG
    unchanged()
    # the resident batch is as it was: the same pass gives the same bits
    model.zero_adapter_grads()
    model.forward_backward_adapters_packed(None, segs)
    assert model.losses() == keep_l and all(np.array_equal(v, model.adapter_grad(s, k)) for (s, k), v in keep_g.items())
    model.close()
    m2 = ra.RecommenderModel(cfg, dtype="fp32", max_rows=ROWS_MAX)                 # no batch
    m2.load_state_dict(P)
    for s in range(4):
        m2.load_adapter(s, adapters[s])
    m2.enable_adapter_training(0.0)
    assert call(m2._h, segs) == ARG
    short = {k: (v.reshape(-1, S).copy()) for k, v in packed.items()}
    for k in short:
        short[k][:, 96:] = 0
    m2.upload_trimmed({k: v.reshape(-1) for k, v in short.items()}, 96)
    assert call(m2._h, segs) == STATE                                              # a trimmed batch is inference-only
    m2.close()
    ft = ra.RecommenderModel(ab.finetune_config(cfg), dtype="fp32", max_rows=ROWS_MAX)
    ft.upload(flat)
    assert call(ft._h, segs) == ARG                                                # a finetune = 1 model owns its adapter
    ft.close()


# ============================================================================================ 7: CLI
def test_cli_finetune_all_pack_writes_files_get_models_serves(tmp_path):
    """`cli --finetune CKPT --finetune_all --finetune_pack` at the tiny size with S = 64 on finetune rows (a live prefix, zeros behind):
    FinetuneDataset -> pack_adapter_rows -> packed joint passes -> the written files -> serve.get_models"""
    from oracle import synth
    from recommendersystem_amd import cli, data, h5, serve, workload
    if not os.path.exists(h5.LIB_PATH):
        pytest.skip("librsys_h5.so not built (no libhdf5 on this host)")
    cfg = workload.make_config("tiny", max_sequence_length=64)
    cfg["lora_dropout"] = 0.1
    Sc = cfg["max_sequence_length"]
    d = str(tmp_path)
    P = synth.make_params(cfg, 5, "test")
    table = P["item_embedding.metadata_embedding.embedding.weight"][:-1]
    h5.write_h5(f"{d}/media_embeddings.h5", {"metadata": table}, blosc=3)
    blob = {"model/" + k: v for k, v in P.items() if "metadata_embedding" not in k}
    blob["config"] = np.frombuffer(json.dumps(cfg).encode(), np.uint8)
    blob["epoch"] = np.array([0])
    np.savez(f"{d}/base_ckpt.npz", **blob)
    rows = 16
    for split, seed in (("training", 1), ("test", 2)):
        stream = {k: np.array(np.asarray(v).reshape(rows, Sc)) for k, v in workload.make_stream(cfg, rows * Sc, seed, mu=np.log(8.0), sigma=0.6).items()}
        live = np.random.default_rng(seed).integers(6, 40, rows)
        for r in range(rows):                                     # one user per row: a live prefix, zeros behind
            for v in stream.values():
                v[r, live[r]:] = 0
            stream["userid"][r, :live[r]] = r + 1
        data.write_shards(f"{d}/transformer/{split}", [[stream]], 1)
    hist = cli.main(["--datadir", d, "--finetune", f"{d}/base_ckpt.npz", "--finetune_all", "--finetune_pack", "--dtype", "fp32",
                     "--local_batch_size", "2", "--global_batch_size", "4", "--num_epochs", "2"])
    assert sorted(hist) == [0, 1, 2, 3]
    assert all(len(hh) >= 1 and np.isfinite([x for _, tr, te in hh for x in (tr, te)]).all() for hh in hist.values())
    out = f"{d}/finetune_all"
    names = ["0.watch", "0.rating", "1.watch", "1.rating"]
    load = lambda p: (lambda z: {k: z[k] for k in z.files})(np.load(p))
    loras = [load(f"{out}/{n}.lora.npz") for n in names]
    for n, lo in zip(names, loras):
        rows_csv = open(f"{out}/{n}.csv").read().strip().split("\n")
        assert rows_csv[0] == "epoch,training_loss,test_loss," + n and rows_csv[1].split(",")[0] == "-1" and len(rows_csv) >= 3
        assert sum("lora_" in k for k in lo) == 4 * cfg["num_layers"]
    assert any(int(lo["epoch"][0]) >= 0 and any(np.abs(v).max() > 0 for k, v in lo.items() if "lora_B" in k) for lo in loras)
    model = serve.get_models(load(f"{out}/base.npz"), loras, dict(cfg, finetune=True), dtype="fp32", max_rows=2)
    model.load_pretrained_embeddings(table)
    assert model.adapters_loaded() == [0, 1, 2, 3]
    model.close()
