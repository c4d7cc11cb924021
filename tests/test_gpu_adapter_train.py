"""GPU: training through the adapter bank (rsys_adapter_train_enable / _forward_backward / _adamw_step) -- the four finetune
adapters on one base model, one slot and task per batch row -- against the fp64 oracle run per adapter on that adapter's rows, against
the existing single-adapter path (a finetune = 1 model with the same tensors on the same rows), and its exact properties.

Batches: oracle.synth rows thinned to at most KEEP targets per row and task.  A finetune row carries few targets (the reference's
FinetuneDataset: one), and only then is "the slot's rows alone" the same problem as "the slot's rows inside a joint batch": the
position selection keeps mask_topk x (rows of the batch) positions per task, so a run on two rows truncates where the joint batch of
six does not.  The set-up asserts that no slot's rows exceed that count and that every slot has a target."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _adapter_bank_util as ab  # noqa: E402

pytestmark = pytest.mark.gpu

CONFIGS = {"tiny": (dict(mask_rate=0.25, mask_topk=6), 26), "hd64": (dict(mask_rate=0.2, mask_topk=16), 21),
           # 2S = 40, D = 80, hd = 16 (base: the shape make_config starts from): the bank's ragged branches inside the whole model -- a half
           # token tile (40 % 16 == 8), a partial token-K step in dA / dB (40 % 32), a partial bf16 K step over the columns (80 % 32 == 16)
           "s20d80": (dict(base="tiny", max_sequence_length=20, embed_dim=80, num_heads=5, num_kv_heads=1, intermediate_dim=224, mask_rate=0.25,
                           mask_topk=6), 20)}
REGULAR = ["tiny", "hd64"]           # the shapes of the tests that need per-shape constants
ROWS = 6
SLOTS = [0, 1, 2, 3, -1, 2]          # slot s runs task s; two rows for slot 2 (accumulation across rows), one base-model row
TASKS = [0, 1, 2, 3, -1, 2]
KEEP = 4
METRICS = ("watch", "rating")
FP32_TOL = 1e-4                      # the project's fp32 bound


def relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _thin(cfg, d, rows):
    """at most KEEP targets per row and task: the later ones lose their weight (inputs only)"""
    S = cfg["max_sequence_length"]
    d = {k: np.array(v) for k, v in d.items()}
    for m in (0, 1):
        for x in METRICS:
            w = d[f"{m}.{x}.weight"].reshape(rows, S)
            for r in range(rows):
                on = np.flatnonzero(w[r] > 0)
                w[r, on[KEEP:]] = 0
            d[f"{m}.{x}.weight"] = w.reshape(d[f"{m}.{x}.weight"].shape)
    return d


def _rows(cfg, d, mine, rows=ROWS):
    S = cfg["max_sequence_length"]
    return {k: np.ascontiguousarray(np.asarray(v).reshape(rows, S)[mine].reshape(-1)) for k, v in d.items()}


def _task_cfg(cfg, task):
    ft = ab.finetune_config(cfg)
    ft.update(finetune_metric=METRICS[task & 1], finetune_medium=task >> 1)
    return ft


_SETUPS = {}


def _setup(name, seed_shift=0):
    """cfg, base parameters, the thinned batch, four adapters; the preconditions of the module docstring asserted"""
    key = (name, seed_shift)
    if key not in _SETUPS:
        from oracle import synth
        over, seed = CONFIGS[name]
        over = dict(over)
        cfg = synth.make_config(over.pop("base", name), **over)
        S, K = cfg["max_sequence_length"], cfg["mask_topk"]
        P = synth.make_params(cfg, seed, "test")
        d = _thin(cfg, synth.make_batch(cfg, ROWS, seed + 1 + seed_shift), ROWS)
        adapters = ab.make_adapters(cfg, 4, seed + 50)
        for s in range(4):
            mine = [r for r in range(ROWS) if SLOTS[r] == s]
            for m in (0, 1):
                for x in METRICS:                 # per task: what one run's selection (mask_topk x its rows) holds
                    n = int((np.asarray(d[f"{m}.{x}.weight"]).reshape(ROWS, S)[mine] > 0).sum())
                    assert n <= K * len(mine), (name, s, m, x, n)
            own = np.asarray(d[f"{s >> 1}.{METRICS[s & 1]}.weight"]).reshape(ROWS, S)[mine]
            assert (own > 0).sum() >= 1, (name, s)
        _SETUPS[key] = (cfg, P, d, adapters)
    return _SETUPS[key]


_ORACLE = {}


def _oracle(name, s, scale=None):
    """losses, weight sum and LoRA gradients of adapter s on its own rows, float64, task s alone (one-hot task_w)"""
    key = (name, s, None if scale is None else tuple(scale))
    if key not in _ORACLE:
        from oracle import model_np
        cfg, P, d, adapters = _setup(name)
        ad = adapters[s] if scale is None else {k: v * np.float32(scale[s]) for k, v in adapters[s].items()}
        mine = [r for r in range(ROWS) if SLOTS[r] == s]
        ft = _task_cfg(cfg, s)
        dm = model_np.mask_tokens(ft, model_np.reshape_batch(ft, _rows(cfg, d, mine)))
        tw = [1.0 if i == s else 0.0 for i in range(4)]
        losses, G = model_np.OracleModel(ft, dict(P, **ad), np.float64).forward(dm, False, True, tw)
        wsum = float(dm[f"{s >> 1}.{METRICS[s & 1]}.weight"].sum())
        assert all(np.abs(G[k]).max() > 0 for k in ad), (name, s, [k for k in ad if np.abs(G[k]).max() == 0])
        _ORACLE[key] = (float(losses[s]), wsum, {k: G[k] for k in ad})
    return _ORACLE[key]


def _bank(name, dtype, dropout=0.0, adapters=None):
    import recommendersystem_amd as ra
    cfg, P, d, ads = _setup(name)
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=ROWS)
    model.load_state_dict(P)
    for s, ad in enumerate(ads if adapters is None else adapters):
        model.load_adapter(s, ad)
    model.enable_adapter_training(dropout)
    return model


def _ft_model_run(name, dtype, s, micro=1):
    """the existing path: a finetune = 1 model of task s holding base + adapter s, on the slot's rows, one-hot task weights"""
    import recommendersystem_amd as ra
    cfg, P, d, adapters = _setup(name)
    mine = [r for r in range(ROWS) if SLOTS[r] == s]
    ft = ra.RecommenderModel(_task_cfg(cfg, s), dtype=dtype, max_rows=len(mine))
    ft.load_state_dict(dict(P, **adapters[s]))
    ft.set_loss_weights([1.0 if i == s else 0.0 for i in range(4)], micro)
    ft.zero_grad()
    sub = _rows(cfg, d, mine)
    for _ in range(micro):
        losses = ft(sub, False)
    out = (losses[s], ft.last_weight_sums[s], {k: ft.grad(k) for k in adapters[s]})
    ft.close()
    return out


def _errors(got, ref):
    """(loss error, weight-sum error, worst gradient error relative to each tensor's maximum)"""
    return (abs(got[0] - ref[0]) / abs(ref[0]), abs(got[1] - ref[1]) / max(abs(ref[1]), 1e-30), max(relerr(got[2][k], ref[2][k]) for k in ref[2]))


def _compare(name, dtype, micro, what):
    bank = _bank(name, dtype)
    cfg, P, d, adapters = _setup(name)
    bank.upload(d)
    bank.zero_adapter_grads()
    for _ in range(micro):
        losses = bank.forward_backward_adapters(None, SLOTS, TASKS, grad_scale=1.0 / micro)
    wsums = bank.last_weight_sums
    eb, eo = [], []
    for s in range(4):
        ref = _oracle(name, s)
        assert ref[0] > 0 and ref[1] > 0
        eb.append(_errors((losses[s], wsums[s], bank.adapter_grad(s)), ref))
        eo.append(_errors(_ft_model_run(name, dtype, s, micro), ref))
    bank.close()
    eb, eo = np.array(eb), np.array(eo)
    print(f"adapter training {what} {name} {dtype}: bank errors per slot (loss, weight sum, gradient) {eb.tolist()}, "
          f"finetune = 1 model {eo.tolist()}")
    if dtype == "fp32":
        assert eb.max() < FP32_TOL, eb
    else:                                           # one figure per quantity: the worst slot, as the bank's inference test takes the worst row
        for q in range(3):
            assert eb[:, q].max() <= 1.5 * eo[:, q].max(), (q, eb[:, q], eo[:, q])
    return losses, wsums


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_parity_per_adapter(name, dtype):
    """Losses, weight sums and every LoRA gradient of slot s against OracleModel(finetune cfg of task s, base + adapter s) in float64
    on that slot's rows alone, and against a finetune = 1 model on the same rows.  fp32: < 1e-4 (gradients relative to each tensor's
    maximum).  bf16: the bank's error <= 1.5 x the finetune model's error against the same oracle, per quantity, worst slot each."""
    losses, wsums = _compare(name, dtype, 1, "parity")
    # the slot -1 row carries no loss: every task's weight sum is that of its slot's rows (checked above against the oracle on those
    # rows alone), and a pass in which ONLY that row keeps its place has no weight and no loss at all
    bank = _bank(name, dtype)
    cfg, P, d, adapters = _setup(name)
    none = bank.forward_backward_adapters(d, [-1] * ROWS, [-1] * ROWS)
    assert none == [0.0] * 4 and bank.last_weight_sums == [0.0] * 4
    assert all(not g.any() for s in range(4) for g in bank.adapter_grad(s).values())
    bank.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_two_micro_steps_accumulate(name, dtype):
    """two passes at grad_scale = 1/2 over the same batch: the oracle's gradient, within the bound of the parity test"""
    _compare(name, dtype, 2, "two micro-steps")


def _grads(bank):
    return {(s, k): v for s in range(5) for k, v in bank.adapter_grad(s).items()}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", REGULAR)
def test_exact_properties(name, dtype):
    from recommendersystem_amd.optim import AdapterAdamW
    cfg, P, d, adapters = _setup(name)
    _, _, d_other, _ = _setup(name, seed_shift=7)
    S = cfg["max_sequence_length"]
    bank = _bank(name, dtype, adapters=adapters + [adapters[0]])      # slot 4: complete, never named by a row
    run = lambda batch, slots, tasks: (bank.zero_adapter_grads(), bank.forward_backward_adapters(batch, slots, tasks, step=3), _grads(bank))[1:]
    l1, g1 = run(d, SLOTS, TASKS)
    l2, g2 = run(d, SLOTS, TASKS)
    assert l1 == l2 and all(np.array_equal(g1[k], g2[k]) for k in g1)                 # a repeated call: equal bits
    assert all(not g1[(4, k)].any() for k in adapters[0])                              # no row, no gradient
    assert all(g1[(s, k)].any() for s in range(4) for k in adapters[s])
    # slot 2 (rows 2 and 5) does not see the other rows: other users there, or no adapter there
    mixed = {k: np.array(v) for k, v in d.items()}
    for k in mixed:
        a, b = mixed[k].reshape(ROWS, S), np.asarray(d_other[k]).reshape(ROWS, S)
        a[[0, 1, 3, 4]] = b[[0, 1, 3, 4]]
        mixed[k] = a.reshape(-1)
    _, g3 = run(mixed, SLOTS, TASKS)
    only = [2 if s == 2 else -1 for s in SLOTS]
    _, g4 = run(d, only, only)
    for k in adapters[2]:
        assert np.array_equal(g1[(2, k)], g3[(2, k)]) and np.array_equal(g1[(2, k)], g4[(2, k)]), k
    assert any(not np.array_equal(g1[(0, k)], g3[(0, k)]) for k in adapters[0])
    # an optimizer step in which slot 4 is inactive leaves its masters, moments and step count bit for bit
    opt = AdapterAdamW(bank, lr=1e-2, slots=range(5))
    rng = np.random.default_rng(5)
    st = {4: {"step": 3, "state": {k: {"exp_avg": rng.standard_normal(v.shape).astype(np.float32),
                                       "exp_avg_sq": rng.random(v.shape).astype(np.float32)} for k, v in adapters[0].items()}}}
    opt.load_state_dict(st)
    before_p, before_o = bank.adapter_state_dict(4), opt.state_dict()[4]
    moved_before = bank.adapter_state_dict(2)
    run(d, SLOTS, TASKS)                                                               # every slot 0 .. 3 has a gradient again
    norms = opt.step({s: 1.0 for s in range(4)}, clip_max_norm=1.0)
    assert all(norms[s] > 0 for s in range(4))
    after_p, after_o = bank.adapter_state_dict(4), opt.state_dict()[4]
    assert after_o["step"] == before_o["step"] == 3 and opt.state_dict()[2]["step"] == 1
    for k in adapters[0]:
        assert np.array_equal(before_p[k], after_p[k])
        assert np.array_equal(before_o["state"][k]["exp_avg"], after_o["state"][k]["exp_avg"])
        assert np.array_equal(before_o["state"][k]["exp_avg_sq"], after_o["state"][k]["exp_avg_sq"])
        assert np.array_equal(st[4]["state"][k]["exp_avg"], after_o["state"][k]["exp_avg"])
    assert any(not np.array_equal(moved_before[k], v) for k, v in bank.adapter_state_dict(2).items())
    assert all(not g.any() for s in range(5) for g in bank.adapter_grad(s).values())  # the step zeroed what it consumed
    bank.close()


# per-adapter scale of the LoRA tensors: by the oracle's norms some slots are clipped at 1.0 and some are not (asserted in the test)
OPT_SCALE = {"tiny": [1.0, 1.0, 0.03, 0.05], "hd64": [1.0, 1.0, 0.005, 0.01]}
OPT_LR = {"tiny": 1e-3, "hd64": 1e-4}


@pytest.mark.parametrize("dtype,tol", [("fp32", 3e-4), ("bf16", 8e-2)])
@pytest.mark.parametrize("name", REGULAR)
def test_three_joint_optimizer_steps(name, dtype, tol):
    """Three joint steps (forward / backward, per-slot clip at 1.0, AdamW) against oracle.train_np's clip_grad_norm and AdamW run per
    adapter on that adapter's rows.  Norms: the bounds of test_clip_adamw_three_steps_vs_golden, the project's three-step optimizer
    test (3e-4 in fp32, 8e-2 in bf16).  Parameters, relative to each tensor's maximum: 3e-4 in fp32 (that test's bound); in bf16 the
    rule of the parity test -- the bank's error against the oracle is at most 1.5 x the error of a finetune = 1 model holding the same
    tensors, stepped three times with AdamW and the same clip on the same rows.  (A fixed bf16 bound has no basis here: AdamW's
    first steps move an element by about lr x sign(gradient), so an element whose gradient lies below the bf16 noise moves by +-lr
    whatever computed it, and on the down-scaled adapters three such steps are a sizeable part of the tensor's maximum.)"""
    import recommendersystem_amd as ra
    from oracle import model_np, train_np
    from recommendersystem_amd.optim import AdamW, AdapterAdamW
    cfg, P, d, adapters = _setup(name)
    scaled = [{k: v * np.float32(OPT_SCALE[name][s]) for k, v in adapters[s].items()} for s in range(4)]
    onehot = lambda s: [1.0 if i == s else 0.0 for i in range(4)]
    ref_P, ref_norms = [], []
    for s in range(4):
        mine = [r for r in range(ROWS) if SLOTS[r] == s]
        ft = _task_cfg(cfg, s)
        dm = model_np.mask_tokens(ft, model_np.reshape_batch(ft, _rows(cfg, d, mine)))
        Ps = {k: np.asarray(v, np.float64) for k, v in dict(P, **scaled[s]).items()}
        names = list(scaled[s])
        opt = train_np.AdamW(Ps, names, OPT_LR[name])
        norms = []
        for _ in range(3):
            _, G = model_np.OracleModel(ft, Ps, np.float64).forward(dm, False, True, onehot(s))
            G, norm = train_np.clip_grad_norm({k: G[k] for k in names}, 1.0)
            Ps = opt.step(dict(Ps), G)
            norms.append(norm)
        ref_P.append(Ps); ref_norms.append(norms)
    print(f"adapter optimizer {name} {dtype}: oracle norms per slot and step {ref_norms}")
    for step in range(3):                                       # in every step one slot is clipped and one is not
        at = [float(n[step]) for n in ref_norms]
        assert max(at) > 1.05 and min(at) < 0.95, (step, at)
    bank = _bank(name, dtype, adapters=scaled)
    opt = AdapterAdamW(bank, lr=OPT_LR[name], slots=range(4))
    bank.upload(d)
    for step in range(3):
        bank.forward_backward_adapters(None, SLOTS, TASKS)
        norms = opt.step({s: 1.0 for s in range(4)}, clip_max_norm=1.0)
        for s in range(4):
            assert abs(norms[s] - ref_norms[s][step]) < tol * ref_norms[s][step], (step, s, norms[s], ref_norms[s][step])
    worst = max(relerr(v, ref_P[s][k]) for s in range(4) for k, v in bank.adapter_state_dict(s).items())
    assert [opt.state_dict()[s]["step"] for s in range(4)] == [3] * 4
    bank.close()
    if dtype == "fp32":
        print(f"adapter optimizer {name} {dtype}: worst parameter error after three steps {worst:.3e}")
        assert worst < tol, worst
        return
    worst_ft = 0.0
    for s in range(4):                                          # the existing path, same tensors, same rows, same three steps
        mine = [r for r in range(ROWS) if SLOTS[r] == s]
        ft = ra.RecommenderModel(_task_cfg(cfg, s), dtype=dtype, max_rows=len(mine))
        ft.load_state_dict(dict(P, **scaled[s]))
        ft.set_loss_weights(onehot(s), 1)
        ft.zero_grad()
        fopt = AdamW(ft, lr=OPT_LR[name])
        sub = _rows(cfg, d, mine)
        for _ in range(3):
            ft(sub, False)
            fopt.step(clip_max_norm=1.0)
        worst_ft = max(worst_ft, max(relerr(ft.get_parameter(k), ref_P[s][k]) for k in scaled[s]))
        fopt.close(); ft.close()
    print(f"adapter optimizer {name} {dtype}: worst parameter error after three steps: bank {worst:.3e}, finetune = 1 model {worst_ft:.3e}")
    assert worst <= 1.5 * worst_ft, (worst, worst_ft)


def test_dropout():
    """fp32, p = 0.5: fresh masks per step, the same (seed, step) bit for bit, evaluation without dropout, and a directional finite
    difference of one lora_A and one lora_B tensor at a fixed (seed, step): the mismatch with dropout may be at most 3 x the mismatch
    of the identical check without it (that path is pinned to the oracle by the parity test; a mask that differs between forward and
    backward is an O(1) mismatch)."""
    name = "tiny"
    cfg, P, d, adapters = _setup(name)
    bank = _bank(name, "fp32", dropout=0.5)
    bank.upload(d)
    fb = lambda step, ev=False: bank.forward_backward_adapters(None, SLOTS, TASKS, evaluate=ev, step=step)
    a = fb(1); ga = _grads_of(bank, 4); bank.zero_adapter_grads()
    b = fb(2); bank.zero_adapter_grads()
    c = fb(1); gc = _grads_of(bank, 4); bank.zero_adapter_grads()
    assert a == c and all(np.array_equal(ga[k], gc[k]) for k in ga)
    assert all(abs(a[i] - b[i]) > 1e-6 * abs(a[i]) for i in range(4)), (a, b)
    ev = fb(1, True)
    bank.enable_adapter_training(0.0)
    assert ev == fb(1, True) and ev == fb(9, True)
    mism = {}
    for p_drop in (0.0, 0.5):
        bank.enable_adapter_training(p_drop)
        for s, key in ((1, "transformers.layers.0.attn.q_proj_lora_A.weight"), (2, "transformers.layers.1.attn.v_proj_lora_B.weight")):
            bank.load_adapter(s, adapters[s])
            bank.zero_adapter_grads()
            f0 = fb(5)[s]
            g = bank.adapter_grad(s, key).astype(np.float64)
            bank.zero_adapter_grads()
            gn = float(np.sqrt((g ** 2).sum()))
            u = g / gn                              # along the computed gradient: the derivative is its norm, as large as a direction gives
            worst = 0.0
            for frac in (0.005, 0.01, 0.02):        # steps that move the loss by about frac of itself; the check keeps the worst of the three
                h = frac * f0 / gn
                f = []
                for sign in (1.0, -1.0):
                    bank.load_adapter(s, dict(adapters[s], **{key: (adapters[s][key] + sign * h * u).astype(np.float32)}))
                    f.append(fb(5)[s])
                    bank.zero_adapter_grads()
                fd = (f[0] - f[1]) / (2 * h)
                worst = max(worst, abs(fd - gn) / gn)
                print(f"adapter dropout p={p_drop} slot {s} {key} h={h:.3e}: finite difference {fd:.6e}, gradient norm {gn:.6e}")
            bank.load_adapter(s, adapters[s])
            mism[(p_drop, key)] = worst
            print(f"adapter dropout p={p_drop} slot {s} {key}: mismatch {worst:.3e}")
    for (p_drop, key), v in mism.items():
        if p_drop > 0:
            assert v <= 3 * mism[(0.0, key)], (key, v, mism[(0.0, key)])
    bank.close()


@pytest.fixture
def dense_top(monkeypatch):
    """RSYS_SPARSE_TOP=0 for the models the test creates; the environment and the parsed switches are restored afterwards"""
    from recommendersystem_amd._lib import lib
    monkeypatch.setenv("RSYS_SPARSE_TOP", "0")
    lib().rsys_switches_reload()
    yield
    monkeypatch.undo()
    lib().rsys_switches_reload()


def test_dropout_matches_the_finetune_model(dense_top):
    """The bank's dropout IS the finetune = 1 model's: both key the mask on (seed ^ 0xD409, step * 64 + layer, element of the layer's
    [tokens][D] LoRA input), the model in a pass of its own (launch_dropout), the bank inside stage A, dA and dx.  A joint pass in which
    every row names slot s at bank dropout 0.5 against the finetune = 1 model of task s with lora_dropout = 0.5 on the same batch, seed and
    step, fp32: the loss and every LoRA gradient within FP32_TOL (gradients relative to each tensor's maximum).
    With the last layer dense (RSYS_SPARSE_TOP=0).  Under the compact top that layer runs in selected-first token order, so ITS element
    index is a token's place in that order, and the order follows the positions the pass selected: the joint pass and the finetune = 1
    model select different sets (other tasks' targets), draw the same mask array and lay it over different tokens of the last layer --
    two equally valid masks, not comparable value for value."""
    import recommendersystem_amd as ra
    name = "tiny"
    cfg, P, d, adapters = _setup(name)
    bank = _bank(name, "fp32", dropout=0.5)
    bank.upload(d)
    for s in range(4):
        bank.zero_adapter_grads()
        plain = bank.forward_backward_adapters(None, [s] * ROWS, [s] * ROWS, evaluate=True, step=5)[s]
        plain = plain[0] if isinstance(plain, list) else plain                    # (a rating task's evaluation: [mse, ...])
        bank.zero_adapter_grads()
        loss = bank.forward_backward_adapters(None, [s] * ROWS, [s] * ROWS, step=5)[s]
        grads = bank.adapter_grad(s)
        assert abs(loss - plain) > 1e-3 * abs(plain), (s, loss, plain)            # the mask acts
        ft = ra.RecommenderModel(dict(_task_cfg(cfg, s), lora_dropout=0.5), dtype="fp32", max_rows=ROWS)
        ft.load_state_dict(dict(P, **adapters[s]))
        ft.set_loss_weights([1.0 if i == s else 0.0 for i in range(4)], 1)
        ft.zero_grad()
        ft.upload(d)
        ft.forward_resident(False, step=5)
        ref_loss = ft.losses()[s]
        ref = {k: ft.grad(k) for k in adapters[s]}
        ft.close()
        e_loss = abs(loss - ref_loss) / abs(ref_loss)
        e_grad = max(relerr(grads[k], ref[k]) for k in ref)
        print(f"adapter dropout 0.5, all rows on slot {s}: loss {loss:.6f} finetune = 1 model {ref_loss:.6f} (rel {e_loss:.2e}), "
              f"worst gradient error {e_grad:.2e}")
        assert e_loss < FP32_TOL and e_grad < FP32_TOL, (s, e_loss, e_grad)
    bank.close()


def _grads_of(bank, n):
    return {(s, k): v for s in range(n) for k, v in bank.adapter_grad(s).items()}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_training_the_bank_leaves_the_model_untouched(dtype):
    """After enabling and training the bank (passes and an optimizer step): state_dict, item table, an rsys_infer_select result and the
    losses and gradients of a following deterministic ordinary training step are bit-equal to a model that never had a bank."""
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd.optim import AdapterAdamW
    name = "hd64"
    cfg, P, d, adapters = _setup(name)
    S = cfg["max_sequence_length"]
    wm, rm = synth.make_masks(cfg, ROWS, 7)
    idx = np.arange(0, ROWS * 2 * S, 5, dtype=np.int32)
    di = dict(d, rope_input_pos=np.tile(np.arange(S, dtype=np.int32), ROWS))
    grads = ["transformers.layers.0.attn.q_proj.weight", "transformers.layers.1.mlp.w2.weight", "item_embedding.projection_layer.weight",
             "item_embedding.matchedid_embedding.embedding.weight", "rating_head.0.weight", "rating_head.2.bias", "norm.scale",
             "transformers.layers.0.sa_norm.scale"]

    def observe(with_bank):
        m = ra.RecommenderModel(dict(cfg, forward="train"), dtype=dtype, max_rows=ROWS)
        m.set_deterministic(True)
        m.load_state_dict(P)
        names = [n for n, _, _ in m.named_parameters()]
        if with_bank:
            for s, ad in enumerate(adapters):
                m.load_adapter(s, ad)
            m.enable_adapter_training(0.1)
            opt = AdapterAdamW(m, lr=1e-2, slots=range(4))
            for step in range(2):
                m.forward_backward_adapters(d, SLOTS, TASKS)
                m.forward_backward_adapters(d, SLOTS, TASKS, evaluate=True)
                opt.step({s: 1.0 for s in range(4)}, clip_max_norm=1.0)
        sd = m.state_dict()
        table = m.item_embeddings()
        sel = m.inference_select(di, "ranking", idx)
        m.set_loss_weights([0.05, 0.2, 0.3, 0.25])
        losses = m({k: v for k, v in d.items()}, False, masks=(wm, rm))      # (no zero_grad in between: nothing may have reached G)
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
    from oracle import synth
    from recommendersystem_amd._lib import lib
    name = "tiny"
    cfg, P, d, adapters = _setup(name)
    Lb, ARG = lib(), -1
    qa = b"transformers.layers.0.attn.q_proj_lora_A.weight"
    i32 = lambda v: np.asarray(v, np.int32)
    call = lambda h, rs, rt: Lb.rsys_adapter_forward_backward(h, 0, None if rs is None else rs.ctypes.data, None if rt is None else rt.ctypes.data,
                                                               1.0, 1, 0)
    ok_s, ok_t = i32(SLOTS), i32(TASKS)
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=ROWS)
    model.load_state_dict(P)
    for s in range(3):
        model.load_adapter(s, adapters[s])
    h = model._h
    buf = np.full(8 * cfg["embed_dim"], -7.25, np.float32)
    model.upload(d)
    assert call(h, ok_s, ok_t) == ARG                                              # training not enabled
    assert Lb.rsys_adapter_grad_get(h, 0, qa, buf.ctypes.data, buf.size) == ARG and (buf == -7.25).all()
    assert Lb.rsys_adapter_zero_grad(h) == ARG
    assert Lb.rsys_adapter_train_enable(h, C.c_float(1.0)) == ARG and Lb.rsys_adapter_train_enable(h, C.c_float(-0.1)) == ARG
    model.enable_adapter_training(0.0)
    assert call(h, ok_s, ok_t) == ARG                                              # slot 3 is not loaded: incomplete
    model.load_adapter(3, adapters[3])
    # a state to keep: gradients of one good pass, the losses it left, the masters
    model.forward_backward_adapters(None, SLOTS, TASKS)
    keep_l, keep_w = model.losses(), list(model.last_weight_sums)
    keep_g = {(s, k): v for s in range(4) for k, v in model.adapter_grad(s).items()}
    keep_p = {(s, k): v for s in range(4) for k, v in model.adapter_state_dict(s).items()}

    def unchanged():
        assert model.losses() == keep_l and list(model.last_weight_sums) == keep_w
        assert all(np.array_equal(v, model.adapter_grad(s, k)) for (s, k), v in keep_g.items())
        assert all(np.array_equal(v, model.adapter_state_dict(s)[k]) for (s, k), v in keep_p.items())

    bad = [(None, ok_t), (ok_s, None),                                             # a null vector
           (i32([0, 1, 2, 3, 8, 2]), ok_t), (i32([0, 1, 2, 3, -2, 2]), ok_t),      # a slot out of range
           (i32([0, 1, 2, 5, -1, 2]), ok_t),                                       # an incomplete (empty) slot
           (ok_s, i32([0, 1, 2, 4, -1, 2])), (ok_s, i32([0, 1, 2, -2, -1, 2])),    # a task out of range
           (ok_s, i32([0, 1, 2, 3, 0, 2])), (ok_s, i32([0, 1, 2, -1, -1, 2])),     # slot -1 with a task, a slot without one
           (i32([0, 1, 2, 3, -1, 0]), ok_t)]                                       # task 2 named by slots 2 and 0
    for rs, rt in bad:
        assert call(h, rs, rt) == ARG, (rs, rt)
        unchanged()
    norms = np.full(4, -7.25, np.float32)
    rec = np.tile(np.float32([1, 1, 1]), (4, 1))
    step = lambda r, n, no: Lb.rsys_adapter_adamw_step(h, C.c_float(1e-2), C.c_float(0.9), C.c_float(0.95), C.c_float(1e-8), C.c_float(0.1),
                                                       None if r is None else r.ctypes.data, n, None if no is None else no.ctypes.data)
    assert step(None, 4, norms) == ARG and step(rec, 4, None) == ARG and step(rec, 0, norms) == ARG and step(rec, 9, norms) == ARG
    rec6 = np.tile(np.float32([1, 1, 1]), (6, 1))                                  # slot 5 is active and empty
    assert step(rec6, 6, np.zeros(6, np.float32)) == ARG
    assert (norms == -7.25).all()
    unchanged()
    assert Lb.rsys_adapter_grad_get(h, 8, qa, buf.ctypes.data, buf.size) == ARG and Lb.rsys_adapter_grad_get(h, 0, qa, buf.ctypes.data, buf.size - 1) == ARG
    assert Lb.rsys_adapter_grad_get(h, 0, b"transformers.layers.0.attn.k_proj_lora_A.weight", buf.ctypes.data, buf.size) == ARG and (buf == -7.25).all()
    model.close()
    # no batch
    m2 = ra.RecommenderModel(cfg, dtype="fp32", max_rows=ROWS)
    m2.load_state_dict(P)
    for s in range(4):
        m2.load_adapter(s, adapters[s])
    m2.enable_adapter_training(0.0)
    assert call(m2._h, ok_s, ok_t) == ARG
    m2.close()
    # a finetune = 1 model owns its adapter; an fp8 model has none
    ft = ra.RecommenderModel(ab.finetune_config(cfg), dtype="fp32", max_rows=ROWS)
    ft.upload(d)
    assert Lb.rsys_adapter_train_enable(ft._h, C.c_float(0.0)) == ARG and call(ft._h, ok_s, ok_t) == ARG
    ft.close()
    cfg8 = synth.make_config("f8t")
    m8 = ra.RecommenderModel(cfg8, dtype="fp8", max_rows=1)
    assert Lb.rsys_adapter_train_enable(m8._h, C.c_float(0.0)) == ARG
    m8.close()
