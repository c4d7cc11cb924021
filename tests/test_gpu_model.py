"""GPU parity tests proper: the HIP path, called through the C ABI via the host mirror of the reference's
model API, against the numpy oracle (itself pinned to the reference, tests/test_oracle_golden.py) and the
committed golden fixtures.  fp32 mode: 1e-4-class tolerances (north_star: logits within 1e-4 relative fp32);
bf16 mode (the benchmarked arithmetic): bf16 tolerances stated per check."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TASK_W = [0.05, 0.2, 0.3, 0.25]


def _setup(name, over, rows, seed, style="test"):
    from oracle import model_np, synth
    cfg = synth.make_config(name, **over)
    P = synth.make_params(cfg, seed, style)
    d = synth.make_batch(cfg, rows, seed + 1)
    return cfg, P, d


def _oracle(cfg, P, d, wm, rm, task_w=TASK_W):
    from oracle import model_np
    ref = model_np.OracleModel(cfg, P, np.float64)
    dm = model_np.mask_tokens(cfg, model_np.reshape_batch(cfg, d), wm, rm)
    y, _ = ref.embed(dm)
    losses, G = ref.forward(dm, False, True, task_w)
    ev = ref.forward(dm, True)
    return y, losses, G, ev


def relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


CASES = [
    ("tiny", dict(mask_rate=0.25, mask_topk=6), 3, 11),
    ("hd64", dict(mask_rate=0.2, mask_topk=16), 2, 23),
]


FWD_BWD_TOLS = [("fp32", 1e-4, 1e-4, 5e-4), ("bf16", 4e-2, 6e-2, 1.5e-1)]


@pytest.mark.parametrize("name,over,rows,seed", CASES)
@pytest.mark.parametrize("dtype,tol_loss,tol_act,tol_grad", FWD_BWD_TOLS)
def test_forward_backward_vs_oracle(name, over, rows, seed, dtype, tol_loss, tol_act, tol_grad):
    _forward_backward_vs_oracle(name, over, rows, seed, dtype, tol_loss, tol_act, tol_grad, False)


@pytest.mark.parametrize("name,over,rows,seed", CASES)
@pytest.mark.parametrize("dtype,tol_loss,tol_act,tol_grad", FWD_BWD_TOLS)
def test_forward_backward_vs_oracle_deterministic(name, over, rows, seed, dtype, tol_loss, tol_act, tol_grad):
    """the same checks in deterministic mode (partial-sum reductions instead of float atomics), with the same bounds"""
    _forward_backward_vs_oracle(name, over, rows, seed, dtype, tol_loss, tol_act, tol_grad, True)


def _forward_backward_vs_oracle(name, over, rows, seed, dtype, tol_loss, tol_act, tol_grad, deterministic):
    import recommendersystem_amd as ra
    from oracle import synth
    cfg, P, d = _setup(name, over, rows, seed)
    z = np.load(os.path.join(GOLDEN, f"model_{name}.npz"))
    u = z["meta/u"]; r = np.float32(cfg["mask_rate"])
    wm = u < r; rm = (u >= r) & (u < 2 * r)
    y_ref, l_ref, G_ref, ev_ref = _oracle(cfg, P, d, wm, rm)
    model = ra.RecommenderModel(dict(cfg, deterministic=deterministic), dtype=dtype, max_rows=rows)
    model.load_state_dict(P)
    model.set_loss_weights(TASK_W, 1)
    losses = model(d, False, masks=(wm, rm))
    y = model.trunk_output(rows)
    assert relerr(y, y_ref) < tol_act, ("trunk", relerr(y, y_ref))
    for a, b in zip(losses, l_ref):
        assert abs(a - b) <= tol_loss * max(abs(b), 1.0), (losses, l_ref)
    # the reference's own numbers (golden fixture), not only the oracle's
    for a, b in zip(losses, z["loss/train"]):
        assert abs(a - b) <= tol_loss * max(abs(b), 1.0), (losses, z["loss/train"])
    gn2 = 0.0
    worst = ("", 0.0)
    for n in synth.trainable_names(cfg):
        g = model.grad(n)
        gn2 += float((g.astype(np.float64) ** 2).sum())
        scale = max(np.abs(G_ref[n]).max(), 1e-3 * np.sqrt((G_ref[n] ** 2).mean()) + 1e-12)
        e = float(np.abs(g - G_ref[n]).max() / max(scale, 1e-6))
        if e > worst[1]:
            worst = (n, e)
    assert worst[1] < tol_grad, worst
    assert abs(np.sqrt(gn2) - z["grad_norm"][0]) < tol_grad * z["grad_norm"][0]
    # evaluate=True: rating entries are the three moments
    ev = model(d, True, masks=(wm, rm))
    flat = []; flat_ref = []
    for a, b in zip(ev, ev_ref):
        flat += a if isinstance(a, list) else [a]
        flat_ref += b if isinstance(b, list) else [b]
    for a, b in zip(flat, flat_ref):
        assert abs(a - b) <= tol_loss * max(abs(b), 1.0), (flat, flat_ref)
    model.close()


@pytest.mark.parametrize("dtype,tol", [("fp32", 3e-4), ("bf16", 8e-2)])
def test_clip_adamw_three_steps_vs_golden(dtype, tol):
    """train.py:259-276 three times on one batch; compared with the reference's own run (fixture)."""
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd.optim import AdamW
    from recommendersystem_amd.train import train_step_unfused
    name, over, rows, seed = CASES[0]
    cfg, P, d = _setup(name, over, rows, seed)
    z = np.load(os.path.join(GOLDEN, f"model_{name}.npz"))
    u = z["meta/u"]; r = np.float32(cfg["mask_rate"])
    wm = u < r; rm = (u >= r) & (u < 2 * r)
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
    model.load_state_dict(P)
    opt = AdamW(model, lr=float(z["opt/lr"][0]))
    for step in range(3):
        losses, norm = train_step_unfused(model, opt, d, list(z["meta/task_w"]), masks=(wm, rm))
        assert relerr(losses, z["opt/losses"][step]) < tol, (step, losses, z["opt/losses"][step])
        assert abs(norm - z["opt/norms"][step]) < tol * z["opt/norms"][step]
    if dtype == "fp32":
        for n in synth.trainable_names(cfg):
            assert relerr(model.get_parameter(n), z["opt/param/" + n]) < tol, n
    model.close()


def test_fused_step_equals_unfused():
    """Fused clip+mean+AdamW (one pass) == clip_grad_norm_ then optimizer.step (train.py:273-275)."""
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd.optim import AdamW
    from recommendersystem_amd.train import train_step_unfused
    name, over, rows, seed = CASES[1]
    cfg, P, d = _setup(name, over, rows, seed)
    wm, rm = synth.make_masks(cfg, rows, 5)
    res = []
    for fused in (False, True):
        model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=rows)
        model.load_state_dict(P)
        opt = AdamW(model, lr=1e-2)
        if fused:
            model.set_loss_weights(TASK_W, 1)
            model(d, False, masks=(wm, rm))
            opt.step(clip_max_norm=1.0, grad_div=1.0)
        else:
            train_step_unfused(model, opt, d, TASK_W, masks=(wm, rm))
        res.append({n: model.get_parameter(n) for n in synth.trainable_names(cfg)})
        g_after = model.grad("transformers.norm.scale")
        if fused:
            assert np.all(g_after == 0)           # optimizer.zero_grad fused
        model.close()
    for n in res[0]:
        assert relerr(res[1][n], res[0][n]) < 5e-4, n   # split-K float atomics: summation order varies run to run, and the first Adam step (m/sqrt(v)) amplifies last-bit gradient differences


def test_grad_accumulation_two_microsteps():
    """no_sync micro-steps (train.py:268-271): two half-batches with grad_accum=2 == sum of scaled grads."""
    import recommendersystem_amd as ra
    from oracle import model_np, synth
    name, over, rows, seed = CASES[1]
    cfg, P, d = _setup(name, over, rows, seed)
    S = cfg["max_sequence_length"]
    wm, rm = synth.make_masks(cfg, rows, 7)
    halves = [({k: v[i * S:(i + 1) * S] for k, v in d.items()}, (wm[i:i + 1], rm[i:i + 1])) for i in range(2)]
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=rows)
    model.load_state_dict(P)
    model.set_loss_weights(TASK_W, 2)
    for dd, mk in halves:
        model(dd, False, masks=mk)
    names = synth.trainable_names(cfg)
    acc = {n: model.grad(n) for n in names}
    ref = {n: 0.0 for n in names}
    for dd, mk in halves:
        o = model_np.OracleModel(cfg, P)
        dm = model_np.mask_tokens(cfg, model_np.reshape_batch(cfg, dd), mk[0], mk[1])
        _, G = o.forward(dm, False, True, [w / 2 for w in TASK_W])
        for n in names:
            ref[n] = ref[n] + G[n]
    worst = max((relerr(acc[n], ref[n]), n) for n in names if np.abs(ref[n]).max() > 1e-8)
    assert worst[0] < 1e-3, worst
    model.close()


def test_grad_accumulation_with_changing_task_weights():
    """A watch head whose task weight is 0 in the first micro-step is skipped there; its first gradient GEMM of the
    second micro-step must ADD to the item-table rows (they already hold the first micro-step's token gradients), not
    store over them (model.hip: gE_clean)."""
    import recommendersystem_amd as ra
    from oracle import model_np, synth
    from recommendersystem_amd.optim import AdamW
    name, over, rows, seed = CASES[1]
    cfg, P, d = _setup(name, over, rows, seed)
    S = cfg["max_sequence_length"]
    wm, rm = synth.make_masks(cfg, rows, 7)
    halves = [({k: v[i * S:(i + 1) * S] for k, v in d.items()}, (wm[i:i + 1], rm[i:i + 1])) for i in range(2)]
    tws = [[0.0, 0.2, 0.0, 0.25], [0.05, 0.2, 0.3, 0.25]]
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=rows)
    model.load_state_dict(P)
    opt = AdamW(model, lr=0.0)
    opt.step()                                   # an optimizer step leaves the gradient rows marked "just zeroed"
    for (dd, mk), tw in zip(halves, tws):
        model.set_loss_weights(tw, 2)
        model(dd, False, masks=mk)
    name_E = "item_embedding.matchedid_embedding.embedding.weight"
    ref = 0.0
    for (dd, mk), tw in zip(halves, tws):
        o = model_np.OracleModel(cfg, P)
        dm = model_np.mask_tokens(cfg, model_np.reshape_batch(cfg, dd), mk[0], mk[1])
        _, G = o.forward(dm, False, True, [w / 2 for w in tw])
        ref = ref + G[name_E]
    assert relerr(model.grad(name_E), ref) < 1e-3
    model.close()


def test_inference_golden():
    """model(d, "retrieval"/"ranking") with rope_input_pos and per-candidate token_mask_ids (fixture from the reference)."""
    import recommendersystem_amd as ra
    from oracle import synth
    z = np.load(os.path.join(GOLDEN, "infer_tiny.npz"))
    cfg = synth.make_config("tiny", mask_rate=0.25, mask_topk=6)
    cfg["forward"] = "inference"
    P = synth.make_params(cfg, 31, "test")
    d = {k[3:]: z[k] for k in z.files if k.startswith("in/")}
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=2)
    model.load_state_dict(P)
    e = model(d, "retrieval")
    assert relerr(e, z["out/retrieval"]) < 1e-4
    r = model(d, "ranking")
    assert relerr(r, z["out/ranking"]) < 1e-4
    model.close()


def test_random_masks_and_properties_at_scale():
    """Size-independent properties at a larger shape (cfg-2-like, bf16): device Philox masks hit the requested
    rate, every padded/zero-weight selected row contributes nothing, loss at reference init ~= ln(V_m),
    two identical steps give the same losses up to float-atomic summation order."""
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config("cfg2", num_layers=2)
    cfg["vocab_sizes"]["0_matchedid"] = 6000; cfg["vocab_sizes"]["1_matchedid"] = 4000
    cfg["metadata_emb_size"] = 100
    rows = 8
    model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=rows)
    model.init_weights(7)
    model.random_pretrained_embeddings(3)
    d = synth.make_batch(cfg, rows, 99)
    model.set_loss_weights(ra.make_task_weights(), 1)
    l1 = model(d, False)
    ws = model.last_weight_sums
    model.zero_grad()
    model.upload(d)
    model.forward_resident(False, step=0)
    model._step = 1
    l2 = model.losses(False)
    # same seed/step -> same masks -> identical losses
    model.zero_grad(); model.forward_resident(False, step=0); l3 = model.losses(False)
    assert relerr(l2, l3) < 1e-5      # same masks; loss sums use float atomics (order-dependent last bits)
    assert abs(l1[0] - np.log(6000)) < 0.05 * np.log(6000) or ws[0] == 0
    assert abs(l1[2] - np.log(4000)) < 0.05 * np.log(4000) or ws[2] == 0
    n = rows * cfg["max_sequence_length"]
    tot_w = sum(float((d[f"{m}.watch.weight"] > 0).sum()) for m in (0, 1))
    assert 0.03 * tot_w < ws[0] + ws[2] < 0.25 * tot_w     # ~mask_rate of the watch targets survive
    for name in ("item_embedding.matchedid_embedding.embedding.weight", "transformers.layers.0.mlp.w1.weight"):
        g = model.grad(name)
        assert np.isfinite(g).all() and np.abs(g).max() > 0
    model.close()


@pytest.mark.parametrize("dtype,tol_loss,tol_act", [("fp32", 1e-4, 1e-4), ("bf16", 4e-2, 6e-2)])
def test_production_sequence_length(dtype, tol_loss, tol_act):
    """The reference's production row is S = 1024 interactions = 2048 tokens (train.py:551): 32 tiles per row, the widest
    the tile bitmaps hold (bit 31 in use), 64-token tiles that straddle users, a row that ends in padding.  Narrow
    model, one row, against the oracle; the second row is all padding (userid 0, no targets)."""
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config("hd64", mask_rate=0.15, mask_topk=160, max_sequence_length=1024, num_layers=1)
    rows, seed = 2, 77
    P = synth.make_params(cfg, seed, "test")
    d = synth.make_batch(cfg, rows, seed + 1, mu=np.log(150.0), sigma=0.7)
    S = cfg["max_sequence_length"]
    for k in d:                                     # row 0: real users, tail padded; row 1: padding only
        d[k][S - 37:] = 0
    wm, rm = synth.make_masks(cfg, rows, seed + 2)
    y_ref, l_ref, G_ref, _ = _oracle(cfg, P, d, wm, rm)
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
    model.load_state_dict(P)
    model.set_loss_weights(TASK_W, 1)
    losses = model(d, False, masks=(wm, rm))
    y = model.trunk_output(rows)
    live = np.zeros(rows * S * 2, bool); live[:2 * (S - 37)] = True      # padded tokens attend among themselves only
    assert relerr(y.reshape(-1, y.shape[-1])[live], y_ref.reshape(-1, y_ref.shape[-1])[live]) < tol_act
    for a, b in zip(losses, l_ref):
        assert abs(a - b) <= tol_loss * max(abs(b), 1.0), (losses, l_ref)
    for n in ("transformers.layers.0.attn.q_proj.weight", "transformers.layers.0.attn.v_proj.weight",
              "item_embedding.matchedid_embedding.embedding.weight"):
        g = model.grad(n)
        scale = max(np.abs(G_ref[n]).max(), 1e-12)
        assert np.abs(g - G_ref[n]).max() / scale < (2e-3 if dtype == "fp32" else 0.2), n
    model.close()


def test_rccl_communicator_world1(monkeypatch):
    """RCCL path on one GPU: ncclCommInitRank(world=1), the bucketed gradient all-reduce and the f64
    all-reduce really call RCCL (RSYS_FORCE_RCCL=1) and leave sums unchanged; hardware_check self test."""
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import dist as rdist
    monkeypatch.setenv("RSYS_FORCE_RCCL", "1")
    name, over, rows, seed = CASES[1]
    cfg, P, d = _setup(name, over, rows, seed)
    wm, rm = synth.make_masks(cfg, rows, 5)
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=rows)
    model.load_state_dict(P)
    model.set_loss_weights(TASK_W, 1)
    model(d, False, masks=(wm, rm))
    before = {n: model.grad(n) for n in ("transformers.layers.0.mlp.w2.weight", "item_embedding.projection_layer.weight")}
    comm = rdist.Comm(rdist.HostGroup(0, 1), 0)
    comm.self_test()
    assert comm.all_reduce_sum([1.5, 2.5]) == [1.5, 2.5]
    comm.all_reduce_grads(model)
    for n, g in before.items():
        np.testing.assert_array_equal(model.grad(n), g)
    comm.close()
    model.close()


def test_rccl_overlapped_table_gradient(monkeypatch):
    """bf16 mode: rsys_allreduce_grads reduces the item-table gradient on the communication stream while the
    metadata-projection gradient GEMM (the last piece of the backward) still runs, then reduces that gradient.  With RCCL
    forced at world 1 every gradient must equal the one of the plain (un-overlapped) finalisation."""
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import dist as rdist
    monkeypatch.setenv("RSYS_FORCE_RCCL", "1")
    name, over, rows, seed = CASES[1]
    cfg, P, d = _setup(name, over, rows, seed)
    wm, rm = synth.make_masks(cfg, rows, 5)
    names = ("item_embedding.projection_layer.weight", "item_embedding.projection_layer.bias",
             "item_embedding.matchedid_embedding.embedding.weight", "transformers.layers.1.attn.q_proj.weight", "transformers.norm.scale")
    grads = []
    for overlapped in (False, True):
        model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=rows)
        model.load_state_dict(P)
        model.set_loss_weights(TASK_W, 1)
        model(d, False, masks=(wm, rm))
        if overlapped:
            comm = rdist.Comm(rdist.HostGroup(0, 1), 0)
            comm.all_reduce_grads(model)
            comm.close()
        grads.append({n: model.grad(n) for n in names})
        model.close()
    for n in names:
        assert relerr(grads[1][n], grads[0][n]) < 1e-5, n


def test_rccl_early_gradient_buckets(monkeypatch):
    """DDP-style bucket hooks (train.py:678-682): armed with rsys_set_grad_sync, the trunk backward starts the all-reduce
    of finished per-layer weight gradients while it is still running, and rsys_allreduce_grads covers the rest exactly
    once.  With RCCL forced at world 1 every gradient must equal the plain path's, the early part must be the trunk's
    weight matrices, and a second (un-armed) step must reduce nothing early."""
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import dist as rdist
    monkeypatch.setenv("RSYS_FORCE_RCCL", "1")
    name, over, rows, seed = CASES[1]
    cfg, P, d = _setup(name, over, rows, seed)
    wm, rm = synth.make_masks(cfg, rows, 5)
    names = synth.trainable_names(cfg)
    grads, early = [], []
    for armed in (False, True):
        model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=rows)
        model.load_state_dict(P)
        model.set_loss_weights(TASK_W, 1)
        comm = rdist.Comm(rdist.HostGroup(0, 1), 0)
        if armed:
            comm.begin_grad_sync(model)
        model(d, False, masks=(wm, rm))
        comm.all_reduce_grads(model)
        early.append(comm.early_reduced(model))
        grads.append({n: model.grad(n) for n in names})
        if armed:                                   # arming lasts for one backward
            model.zero_grad()
            model(d, False, masks=(wm, rm))
            comm.all_reduce_grads(model)
            assert comm.early_reduced(model) == 0
            for n in names:
                assert relerr(model.grad(n), grads[0][n]) < 1e-5, n
        comm.close()
        model.close()
    D, I, L = cfg["embed_dim"], cfg["intermediate_dim"], cfg["num_layers"]
    Ip = (I + 15) // 16 * 16
    nqkv = (cfg["num_heads"] + 2 * cfg["num_kv_heads"]) * (D // cfg["num_heads"])
    assert early[0] == 0 and early[1] >= L * (nqkv * D + D * D + 2 * I * D + D * I), early
    for n in names:
        assert relerr(grads[1][n], grads[0][n]) < 1e-5, n


@pytest.mark.parametrize("dtype,tol_loss,tol_grad", [("fp32", 1e-4, 1e-3), ("bf16", 4e-2, 0.2)])
def test_finetune_lora_golden(dtype, tol_loss, tol_grad):
    """LoRA finetune (model.py:235-271,361-371,418-435): frozen base, rank-8 updates on q and v,
    masks derived from the chosen metric's weights; losses and LoRA gradients against the reference's own run."""
    import recommendersystem_amd as ra
    from oracle import synth
    z = np.load(os.path.join(GOLDEN, "finetune_tiny.npz"))
    cfg = synth.make_config("tiny", mask_rate=0.25, mask_topk=6, finetune=True, finetune_metric="rating")
    cfg["lora_dropout"] = 0.0          # the fixture was generated with the dropout modules in eval()
    P = synth.make_params(cfg, 41, "test")
    d = {k[3:]: z[k] for k in z.files if k.startswith("in/")}
    rows = d["userid"].shape[0]
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
    model.load_state_dict(P)
    names = [n for n, _, tr in model.named_parameters() if tr]
    assert names and all("lora_" in n for n in names)          # everything else is frozen
    model.set_loss_weights([0.0, 1.0, 0.0, 0.5], 1)
    losses = model(d, False)
    for a, b in zip(losses, z["loss/train"]):
        assert abs(a - b) <= tol_loss * max(abs(b), 1.0), (losses, z["loss/train"])
    for k in [k for k in z.files if k.startswith("grad/")]:
        g = model.grad(k[5:])
        ref = z[k]
        assert relerr(g, ref) < tol_grad or np.abs(ref).max() < 1e-7, (k, relerr(g, ref))
    # optimizer touches the LoRA tensors only
    from recommendersystem_amd.optim import AdamW
    opt = AdamW(model, lr=1e-2)
    before = model.get_parameter("transformers.layers.0.mlp.w1.weight")
    a_before = model.get_parameter("transformers.layers.0.attn.q_proj_lora_A.weight")
    opt.step(clip_max_norm=1.0)
    np.testing.assert_array_equal(model.get_parameter("transformers.layers.0.mlp.w1.weight"), before)
    assert np.abs(model.get_parameter("transformers.layers.0.attn.q_proj_lora_A.weight") - a_before).max() > 0
    model.close()


def test_finetune_dropout_runs():
    """nn.Dropout(0.1) on the LoRA input: active in training passes only, fresh mask per step, same mask in backward."""
    import recommendersystem_amd as ra
    from oracle import synth
    z = np.load(os.path.join(GOLDEN, "finetune_tiny.npz"))
    cfg = synth.make_config("tiny", mask_rate=0.25, mask_topk=6, finetune=True, finetune_metric="rating")
    P = synth.make_params(cfg, 41, "test")
    for k in P:
        if "lora_B" in k:
            P[k] = (np.random.default_rng(1).standard_normal(P[k].shape) * 0.3).astype(np.float32)
    d = {k[3:]: z[k] for k in z.files if k.startswith("in/")}
    rows = d["userid"].shape[0]
    res = {}
    for p_drop in (0.0, 0.5):
        cfg["lora_dropout"] = p_drop
        model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=rows)
        model.load_state_dict(P)
        model.set_loss_weights([0.0, 1.0, 0.0, 0.5], 1)
        l_train = [model(d, False)[1] for _ in range(2)]
        l_eval = model(d, True)[1][0]
        g = model.grad("transformers.layers.0.attn.q_proj_lora_A.weight")
        assert np.isfinite(g).all()
        res[p_drop] = (l_train, l_eval)
        model.close()
    assert res[0.0][0][0] == pytest.approx(res[0.0][0][1], rel=1e-6)       # no dropout: repeatable
    assert abs(res[0.5][0][0] - res[0.5][0][1]) > 1e-6                      # fresh mask every step
    assert res[0.5][1] == pytest.approx(res[0.0][1], rel=1e-5)             # evaluate: dropout off


@pytest.mark.parametrize("kern", ["2", "3"])
def test_forward_backward_with_256_tile_gemm(monkeypatch, kern):
    """Same parity check with every eligible row-major bf16 GEMM forced onto the 256x256 LDS-DMA kernel
    (gemm8p.hip; by default it takes over only at >= 128 tiles): fused RoPE / SwiGLU / residual / GELU epilogues,
    ragged M and N, the minimum K depth of its pipeline."""
    monkeypatch.setenv("RSYS_GEMM_KERNEL", kern)
    monkeypatch.setenv("RSYS_GEMM_KERNEL_TN", "2")   # weight gradients on the K-major LDS-DMA kernel too
    name, over, rows, seed = CASES[1]
    test_forward_backward_vs_oracle(name, over, rows, seed, "bf16", 4e-2, 6e-2, 1.5e-1)


def test_resume_from_reference_checkpoint():
    """the reference's own checkpoint (torch pickle written after two steps by its model / AdamW,
    tests/golden/checkpoint_tiny.pt) -> `recommendersystem_amd.checkpoint.from_reference` (committed result) -> resume -> the third step must
    land on the parameters the reference reached (model_tiny.npz opt/param)."""
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd.optim import AdamW
    from recommendersystem_amd.train import load_checkpoint, train_step_unfused
    name, over, rows, seed = CASES[0]
    cfg, P, d = _setup(name, over, rows, seed)
    z = np.load(os.path.join(GOLDEN, f"model_{name}.npz"))
    u = z["meta/u"]; r = np.float32(cfg["mask_rate"])
    wm = u < r; rm = (u >= r) & (u < 2 * r)
    # checkpoint_tiny_converted.npz = checkpoint.from_reference(checkpoint_tiny.pt); the CPU suite checks that equality, so this
    # test needs no torch on the GPU box
    path = os.path.join(GOLDEN, "checkpoint_tiny_converted.npz")
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=rows)
    model.init_weights(1)                                   # whatever: everything trainable comes from the checkpoint
    model.load_pretrained_embeddings(P["item_embedding.metadata_embedding.embedding.weight"][:-1])
    opt = AdamW(model, lr=float(z["opt/lr"][0]))
    epoch, config = load_checkpoint(path, model, opt)
    assert epoch == 1 and config["embed_dim"] == cfg["embed_dim"]
    losses, norm = train_step_unfused(model, opt, d, list(z["meta/task_w"]), masks=(wm, rm))
    assert relerr(losses, z["opt/losses"][2]) < 3e-4, (losses, z["opt/losses"][2])
    assert abs(norm - z["opt/norms"][2]) < 3e-4 * z["opt/norms"][2]
    for n in synth.trainable_names(cfg):
        assert relerr(model.get_parameter(n), z["opt/param/" + n]) < 3e-4, n
    model.close()


def test_hdf5_shards_and_embeddings_feed_the_step(tmp_path):
    """a blosc-3 HDF5 shard (transformer.jl:228-231) read back through PretrainDataset's loader and
    media_embeddings.h5 loaded by directory (model.py:379-389) give the step the same bits as the arrays themselves."""
    import recommendersystem_amd as ra
    from recommendersystem_amd import data, h5
    if not os.path.exists(h5.LIB_PATH):
        pytest.skip("librsys_h5.so not built (no libhdf5 on this host)")
    name, over, rows, seed = CASES[0]
    cfg, P, d = _setup(name, over, rows, seed)
    table = P["item_embedding.metadata_embedding.embedding.weight"][:-1]
    data.write_shards(str(tmp_path / "training"), [[d]], 1, fmt="h5")
    h5.write_h5(str(tmp_path / "media_embeddings.h5"), {"metadata": table}, blosc=3)
    ds = data.PretrainDataset(str(tmp_path / "training"), 0, 1, len(d["userid"]))
    assert [os.path.basename(f) for f in ds.fns] == ["1.h5"]
    got = data.load_shard(ds.fns[0])
    assert sorted(got) == sorted(d) and all(got[k].dtype == d[k].dtype and np.array_equal(got[k], d[k]) for k in d)
    out = []
    for batch, tab in ((d, table), (got, str(tmp_path))):
        model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=rows)
        model.load_state_dict(P)
        model.load_pretrained_embeddings(tab)
        model.set_loss_weights(TASK_W)
        model.zero_grad()
        out.append((model(batch, False), model.grad("item_embedding.projection_layer.weight")))
        model.close()
    assert relerr(out[1][0], out[0][0]) < 1e-6          # fp32 atomics (loss sums, split-K): summation order differs run to run
    assert relerr(out[1][1], out[0][1]) < 1e-5
    assert np.isfinite(out[0][0]).all() and np.abs(out[0][1]).max() > 0


def test_cli_trains_from_a_data_directory(tmp_path):
    """the command line of transformer.py over a data directory in the reference's layout (csv files,
    list_tag, blosc HDF5 shards + num_tokens.txt, media_embeddings.h5): two epochs at a tiny size, the metrics CSV in the
    reference's format, a checkpoint, and a resumed --prod run that continues after the last epoch."""
    from recommendersystem_amd import cli, data, h5, workload
    if not os.path.exists(h5.LIB_PATH):
        pytest.skip("librsys_h5.so not built (no libhdf5 on this host)")
    cfg = workload.make_config("tiny")
    V0, V1, S, M = cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"], cfg["max_sequence_length"], cfg["metadata_emb_size"]
    d = str(tmp_path)
    open(f"{d}/manga.csv", "w").write("matchedid\n" + "\n".join(str(i) for i in range(V0)) + "\n")
    open(f"{d}/anime.csv", "w").write("matchedid\n" + "\n".join(str(i) for i in range(V1)) + "\n")
    open(f"{d}/list_tag", "w").write("20260101")
    cfg["max_ts"] = __import__("datetime").datetime(2026, 1, 1).timestamp()
    rows_per_batch = 4
    for split, nb, seed in (("training", 6, 1), ("test", 2, 2)):
        stream = workload.make_stream(cfg, nb * rows_per_batch * S, seed, mu=np.log(8.0), sigma=0.6)
        data.write_shards(f"{d}/transformer/{split}", [[stream]], 1, fmt="h5")
    table = np.random.default_rng(3).standard_normal((V0 + V1, M)).astype(np.float32) / np.sqrt(M)
    h5.write_h5(f"{d}/media_embeddings.h5", {"metadata": table}, blosc=3)
    argv = ["--datadir", d, "--model", "tiny", "--metadata_emb_size", str(M), "--dtype", "fp32", "--local_batch_size", str(rows_per_batch),
            "--global_batch_size", str(2 * rows_per_batch), "--num_epochs", "2", "--warmup_steps", "2", "--prod"]
    hist = cli.main(argv)
    assert [e for e, _, _ in hist] == [0, 1] and all(np.isfinite(l).all() for _, tr, te in hist for l in (tr, te))
    lines = open(f"{d}/transformer.masked.csv").read().strip().split("\n")
    assert lines[0] == "epoch,training_loss,test_loss,0.watch,0.rating,1.watch,1.rating" and [l.split(",")[0] for l in lines[1:]] == ["-1", "0", "1"]
    assert os.path.exists(f"{d}/transformer.masked.finished")
    saved = os.path.exists(f"{d}/transformer.masked.npz")   # written when the early stopper saw the test loss improve
    argv[argv.index("--num_epochs") + 1] = "3"
    hist2 = cli.main(argv)                                   # --prod resumes after the checkpointed epoch, else starts over
    assert hist2[-1][0] == 2 and (hist2[0][0] > 0) == saved


def test_registry_export_matches_the_item_embedding(tmp_path):
    """Finetune/register.py:14-36: `model.registry.h5` holds ItemEmbedding.forward over every item, split by medium, and the
    rating offsets -- checked against the oracle's fused table (fp32 1e-5, bf16 table arithmetic 2e-2)."""
    import recommendersystem_amd as ra
    from oracle import model_np
    from recommendersystem_amd import h5, serve
    if not os.path.exists(h5.LIB_PATH):
        pytest.skip("librsys_h5.so not built (no libhdf5 on this host)")
    name, over, rows, seed = CASES[1]
    cfg, P, d = _setup(name, over, rows, seed)
    n0, n1 = cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"]
    ref = model_np.OracleModel(cfg, P, np.float64).fused_table()[:n0 + n1]
    for dtype, tol in (("fp32", 1e-5), ("bf16", 2e-2)):
        model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
        model.load_state_dict(P)
        path = str(tmp_path / f"model.registry.{dtype}.h5")
        serve.register_transformer(model, path)
        model.close()
        got = h5.read_h5(path)
        assert sorted(got) == ["0.rating_mean", "0.watch.weight", "1.rating_mean", "1.watch.weight"]
        assert got["0.watch.weight"].shape == (n0, cfg["embed_dim"]) and got["1.watch.weight"].shape == (n1, cfg["embed_dim"])
        assert got["0.rating_mean"].shape == () and float(got["1.rating_mean"]) == pytest.approx(cfg["rating_mean"])
        assert relerr(np.concatenate([got["0.watch.weight"], got["1.watch.weight"]]), ref) < tol, dtype


def test_serving_predict_end_to_end():
    """Request -> response through `serve.predict` (embed.py:74-161) on the HIP inference forward: retrieval returns the
    trunk output at the query item token, ranking the rating head at each candidate's action token; compared with the
    oracle on the batch the same host code built.  Also: a candidate's score must not depend on the other candidates."""
    import recommendersystem_amd as ra
    from oracle import model_np, synth
    from recommendersystem_amd import serve
    cfg = synth.make_config("tiny", mask_rate=0.25, mask_topk=6)
    cfg["forward"] = "inference"
    S = cfg["max_sequence_length"]
    P = synth.make_params(cfg, 31, "test")
    rng = np.random.default_rng(9)

    def user(n_events, cands):
        items, ts = [], 1.2e9
        for _ in range(n_events):
            ts += float(rng.integers(10, 10 ** 6))
            items.append({"medium": int(rng.integers(0, 2)), "matchedid": int(rng.integers(1, 25)), "history_max_ts": ts,
                          "status": int(rng.integers(0, 9)), "rating": float(rng.integers(0, 11)), "progress": float(rng.random()),
                          "history_status": -1, "history_rating": -1.0})
        return {"user": {"gender": None, "source": 2}, "items": items, "timestamp": ts + 60.0, "ranking_items": cands}

    users = [user(5, [3, 7, 11]), user(S, [4, 9])]            # the second history overflows and is truncated
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=2)
    model.load_state_dict(P)
    ref = model_np.OracleModel(cfg, P, np.float64)
    for task, medium in (("retrieval", 1), ("ranking", 0)):
        got = serve.predict(model, users, task, medium)
        mul, mri = (S, 0) if task == "retrieval" else (S // 2, S - S // 2)
        d = serve.build_batch(users, task, medium, cfg["vocab_sizes"]["0_matchedid"], mul, mri)
        exp = serve.extract(ref.inference({k: np.asarray(v) for k, v in d.items()}, task), users, task, medium, mul)
        for g, e in zip(got, exp):
            k = f"{medium}.{task}"
            assert relerr(np.array(g[k]), np.array(e[k])) < 1e-4, (task, g[k], e[k])
    # ranking: candidates are isolated from each other by their token_mask_ids
    a = serve.predict(model, [users[0]], "ranking", 0)[0]["0.ranking"]
    solo = dict(users[0]); solo["ranking_items"] = [users[0]["ranking_items"][1]]
    b = serve.predict(model, [solo], "ranking", 0)[0]["0.ranking"]
    assert abs(a[1] - b[0]) < 1e-4 * max(1.0, abs(a[1]))
    model.close()


def test_full_size_cfg3_parity_and_properties():
    """At BASELINE's full model size (cfg-3: D=512, L=8, S=512, 200 K items, M=6148).
    (1) fp32 mode, one row: trunk output against the fp64 oracle at 1e-4 (the oracle gets the fused item-table rows the row
        uses, computed on the host from the same parameters -- the full 200 K x 6148 projection is not needed for one row);
    (2) bf16 mode, 4 rows: user isolation (changing one user's events leaves every other user's outputs bit-identical:
        the document mask, model.py:479-487) and row-permutation equivariance of the forward."""
    import recommendersystem_amd as ra
    from oracle import model_np, synth
    cfg = synth.make_config("cfg3")
    S, D, M = cfg["max_sequence_length"], cfg["embed_dim"], cfg["metadata_emb_size"]
    V0, V1 = cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"]
    V = V0 + V1
    rng = np.random.default_rng(17)
    base = (rng.standard_normal((997, M)) / np.sqrt(M)).astype(np.float32)
    table = base[np.arange(V) % 997] * (1.0 + (np.arange(V) % 13)[:, None].astype(np.float32) / 13.0)   # (V, M), cheap to rebuild per row

    # ---- (1) fp32, one row, vs oracle
    d = synth.make_batch(cfg, 1, 123, mu=4.6, sigma=1.0)
    wm, rm = synth.make_masks(cfg, 1, 7)
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=1)
    model.init_weights(5)
    for n, shape, tr in model.named_parameters():            # init leaves norm scales at 1 and phases at 0: perturb them
        if tr and (n.endswith(".scale") or "periodic_time" in n):
            model.set_parameter(n, (1.0 if n.endswith(".scale") else 0.0) + 0.1 * rng.standard_normal(shape).astype(np.float32))
    model.load_pretrained_embeddings(table)
    model.set_loss_weights(TASK_W, 1)
    model(d, False, masks=(wm, rm))
    y = model.trunk_output(1)
    P = model.state_dict(include_frozen=False)
    P = {k: v for k, v in P.items() if not k.startswith("watch_head.")}
    dm = model_np.mask_tokens(cfg, model_np.reshape_batch(cfg, d), wm, rm)
    ids = np.unique(np.where(dm["matchedid"] == -1, V, dm["matchedid"]))
    E = P["item_embedding.matchedid_embedding.embedding.weight"].astype(np.float64)
    Wp = P["item_embedding.projection_layer.weight"].astype(np.float64); bp = P["item_embedding.projection_layer.bias"].astype(np.float64)
    meta = np.zeros((len(ids), M), np.float64)
    meta[ids < V] = table[ids[ids < V]]                     # the mask row V has zero metadata (model.py:386)
    F = np.zeros((V + 1, D), np.float64)
    F[ids] = E[ids] + meta @ Wp.T + bp
    P64 = {k: v.astype(np.float64) for k, v in P.items() if "matchedid_embedding" not in k}
    P64["item_embedding.fused_embedding"] = F
    P64["item_embedding.matchedid_embedding.embedding.weight"] = E
    ref = model_np.OracleModel(cfg, P64, np.float64)
    y_ref, _ = ref.embed(dm)
    assert relerr(y, y_ref) < 1e-4, relerr(y, y_ref)
    model.close()

    # ---- (2) bf16, 4 rows: isolation and permutation
    rows = 4
    d = synth.make_batch(cfg, rows, 321, mu=4.6, sigma=1.0)
    wm, rm = synth.make_masks(cfg, rows, 9)
    model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=rows)
    model.init_weights(5)
    model.load_pretrained_embeddings(table)
    model.set_loss_weights(TASK_W, 1)
    model(d, True, masks=(wm, rm))
    y0 = model.trunk_output(rows).copy()
    uid = np.asarray(d["userid"]).reshape(rows, S)
    victim = uid[1, S // 2]
    sel = (uid == victim)
    assert sel.any() and not sel.all()
    d2 = {k: np.array(v, copy=True) for k, v in d.items()}
    flat = sel.reshape(-1)
    d2["rating"] = np.where(flat, 10.0 - np.asarray(d["rating"]).reshape(-1), np.asarray(d["rating"]).reshape(-1)).astype(np.float32)
    d2["status"] = np.where(flat, (np.asarray(d["status"]).reshape(-1) + 3) % 9, np.asarray(d["status"]).reshape(-1)).astype(np.int32)
    mid = np.asarray(d["matchedid"]).reshape(-1)
    d2["matchedid"] = np.where(flat, (mid + 17) % V, mid).astype(np.int32)
    model(d2, True, masks=(wm, rm))
    y1 = model.trunk_output(rows)
    tok = np.repeat(sel, 2, axis=1)                          # tokens of the victim user (item + action per event)
    assert np.array_equal(y0[~tok], y1[~tok])                # everybody else: bit-identical
    assert np.abs(y0[tok] - y1[tok]).max() > 1e-3            # the victim's own outputs moved
    perm = np.array([2, 0, 3, 1])
    dp = {k: np.asarray(v).reshape(rows, S)[perm].reshape(-1) for k, v in d.items()}
    model(dp, True, masks=(wm[perm], rm[perm]))
    yp = model.trunk_output(rows)
    assert np.array_equal(yp, y0[perm])
    model.close()


def test_bench_shape_forward_is_reproducible_and_matches_small_batch():
    """The benchmarked shape (cfg-3, 64 rows: every trunk GEMM on the 256x256 LDS-DMA kernel, whose correctness rests on
    counted waits -- a race shows up as run-to-run differences under memory load).  Three forward passes must give
    bit-identical trunk outputs, and a row must agree with the same row run in a 4-row batch (there the trunk GEMMs take
    the 128x128 kernel: other tiling and summation order, so agreement is to bf16 rounding, not bitwise)."""
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config("cfg3")
    S = cfg["max_sequence_length"]
    rows = 64
    d = synth.make_batch(cfg, rows, 0xD47A, mu=4.6, sigma=1.0)
    wm, rm = synth.make_masks(cfg, rows, 11)
    model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=rows)
    model.init_weights(0x1217)
    model.random_pretrained_embeddings(0x3E7A)
    model.set_loss_weights(TASK_W, 1)
    outs = []
    for _ in range(3):
        model(d, True, masks=(wm, rm))
        outs.append(model.trunk_output(rows).copy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert np.isfinite(outs[0]).all()
    sub = {k: np.asarray(v).reshape(rows, S)[8:12].reshape(-1) for k, v in d.items()}
    model(sub, True, masks=(wm[8:12], rm[8:12]))
    small = model.trunk_output(4)
    assert relerr(small, outs[0][8:12]) < 3e-2, relerr(small, outs[0][8:12])
    model.close()


@pytest.mark.parametrize("name,over,rows,seed", CASES)
def test_bf16_mode_vs_oracle_with_bf16_rounded_operands(name, over, rows, seed):
    """The benchmarked arithmetic against the oracle run with the SAME storage roundings (every bf16 GEMM operand of the
    HIP path rounded to bfloat16 at the point the kernels store it, fp64 accumulation): what is left is summation
    order and the flash kernels' running-maximum rescaling, so the tolerances are 4-10x tighter than bf16-vs-fp64."""
    import recommendersystem_amd as ra
    from oracle import model_np, synth
    cfg, P, d = _setup(name, over, rows, seed)
    wm, rm = synth.make_masks(cfg, rows, seed + 2)
    ref = model_np.OracleModel(cfg, P, np.float64, operand_round="bf16")
    dm = model_np.mask_tokens(cfg, model_np.reshape_batch(cfg, d), wm, rm)
    y_ref, _ = ref.embed(dm)
    l_ref, G_ref = ref.forward(dm, False, True, TASK_W)
    model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=rows)
    model.load_state_dict(P)
    model.set_loss_weights(TASK_W, 1)
    losses = model(d, False, masks=(wm, rm))
    y = model.trunk_output(rows)
    e_y = relerr(y, y_ref)
    e_l = max(abs(a - b) / max(abs(b), 1.0) for a, b in zip(losses, l_ref))
    worst = ("", 0.0)
    for n in synth.trainable_names(cfg):
        g = model.grad(n)
        scale = max(np.abs(G_ref[n]).max(), 1e-3 * np.sqrt((G_ref[n] ** 2).mean()) + 1e-12)
        e = float(np.abs(g - G_ref[n]).max() / max(scale, 1e-6))
        if e > worst[1]:
            worst = (n, e)
    print(f"bf16-vs-bf16-oracle[{name}]: trunk {e_y:.2e} losses {e_l:.2e} worst grad {worst}")
    assert e_y < 1e-2, e_y                       # measured 4e-3 / 6e-3
    assert e_l < 5e-3, (losses, l_ref)           # measured 2e-4 / 2e-3
    assert worst[1] < 5e-2, worst                # measured 3e-2 (a phase parameter with a tiny gradient)
    model.close()


@pytest.mark.parametrize("dtype,tol_loss,tol_act,tol_grad", [("fp32", 1e-4, 1e-4, 5e-4), ("bf16", 4e-2, 6e-2, 1.5e-1)])
def test_cfg1_exact_shape_full_parity(dtype, tol_loss, tol_act, tol_grad):
    """BASELINE configs[0] at its exact shape (cfg-1: D=64, heads 4/2 of 16, I=176, L=2, S=32, 400+600 items, M=6148,
    K=8, 64 rows): trunk output, the four losses and EVERY named gradient against the fp64 oracle."""
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config("cfg1")
    assert (cfg["embed_dim"], cfg["num_heads"], cfg["num_kv_heads"], cfg["intermediate_dim"], cfg["num_layers"],
            cfg["max_sequence_length"], cfg["metadata_emb_size"], cfg["mask_topk"]) == (64, 4, 2, 176, 2, 32, 6148, 8)
    rows, seed = 64, 101
    P = synth.make_params(cfg, seed, "test")
    d = synth.make_batch(cfg, rows, seed + 1)
    wm, rm = synth.make_masks(cfg, rows, seed + 2)
    y_ref, l_ref, G_ref, ev_ref = _oracle(cfg, P, d, wm, rm)
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
    model.load_state_dict(P)
    model.set_loss_weights(TASK_W, 1)
    losses = model(d, False, masks=(wm, rm))
    assert relerr(model.trunk_output(rows), y_ref) < tol_act
    for a, b in zip(losses, l_ref):
        assert abs(a - b) <= tol_loss * max(abs(b), 1.0), (losses, l_ref)
    worst = ("", 0.0)
    for n in synth.trainable_names(cfg):
        g = model.grad(n)
        scale = max(np.abs(G_ref[n]).max(), 1e-3 * np.sqrt((G_ref[n] ** 2).mean()) + 1e-12)
        e = float(np.abs(g - G_ref[n]).max() / max(scale, 1e-6))
        if e > worst[1]:
            worst = (n, e)
    assert worst[1] < tol_grad, worst
    ev = model(d, True, masks=(wm, rm))
    flat = []; flat_ref = []
    for a, b in zip(ev, ev_ref):
        flat += a if isinstance(a, list) else [a]
        flat_ref += b if isinstance(b, list) else [b]
    for a, b in zip(flat, flat_ref):
        assert abs(a - b) <= tol_loss * max(abs(b), 1.0), (flat, flat_ref)
    model.close()


def test_full_size_cfg2_parity_and_properties():
    """BASELINE configs[1] at FULL size (cfg-2: D=256, L=8, S=256, 60 K + 40 K items, M=6148, K=32).
    (1) fp32 mode, 2 rows: trunk output, the four losses, and the gradients of the trunk / rating-head weights against
        the fp64 oracle, which gets the full fused item table (100 001 x 256) computed on the host in fp64 from the same
        parameters and metadata;
    (2) bf16 mode, 4 rows: user isolation and row-permutation equivariance, bit-exact (model.py:479-487)."""
    import recommendersystem_amd as ra
    from oracle import model_np, synth
    cfg = synth.make_config("cfg2")
    S, D, M = cfg["max_sequence_length"], cfg["embed_dim"], cfg["metadata_emb_size"]
    V0, V1 = cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"]
    V = V0 + V1
    assert (D, cfg["num_layers"], S, V, M, cfg["mask_topk"]) == (256, 8, 256, 100000, 6148, 32)
    rng = np.random.default_rng(29)
    base = (rng.standard_normal((997, M)) / np.sqrt(M)).astype(np.float32)
    table = base[np.arange(V) % 997] * (1.0 + (np.arange(V) % 13)[:, None].astype(np.float32) / 13.0)

    # ---- (1) fp32, 2 rows, vs oracle incl. heads and gradients
    rows = 2
    d = synth.make_batch(cfg, rows, 211, mu=4.0, sigma=0.8)
    wm, rm = synth.make_masks(cfg, rows, 13)
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=rows)
    model.init_weights(9)
    for n, shape, tr in model.named_parameters():            # init leaves norm scales at 1 and phases / biases at 0: perturb them
        if tr and (n.endswith(".scale") or "periodic_time" in n or n.endswith(".bias")):
            model.set_parameter(n, (1.0 if n.endswith(".scale") else 0.0) + 0.1 * rng.standard_normal(shape).astype(np.float32))
    model.load_pretrained_embeddings(table)
    model.set_loss_weights(TASK_W, 1)
    losses = model(d, False, masks=(wm, rm))
    y = model.trunk_output(rows)
    P = {k: v for k, v in model.state_dict(include_frozen=False).items() if not k.startswith("watch_head.")}
    E = P["item_embedding.matchedid_embedding.embedding.weight"].astype(np.float64)
    Wp = P["item_embedding.projection_layer.weight"].astype(np.float64); bp = P["item_embedding.projection_layer.bias"].astype(np.float64)
    F = np.empty((V + 1, D), np.float64)
    for r0 in range(0, V, 8192):
        r1 = min(V, r0 + 8192)
        F[r0:r1] = E[r0:r1] + table[r0:r1].astype(np.float64) @ Wp.T + bp
    F[V] = E[V] + bp                                         # the mask row has zero metadata (model.py:386)
    P64 = {k: v.astype(np.float64) for k, v in P.items()}
    P64["item_embedding.fused_embedding"] = F
    ref = model_np.OracleModel(cfg, P64, np.float64)
    dm = model_np.mask_tokens(cfg, model_np.reshape_batch(cfg, d), wm, rm)
    y_ref, _ = ref.embed(dm)
    assert relerr(y, y_ref) < 1e-4, relerr(y, y_ref)
    l_ref, G_ref = ref.forward(dm, False, True, TASK_W)
    for a, b in zip(losses, l_ref):
        assert abs(a - b) <= 1e-4 * max(abs(b), 1.0), (losses, l_ref)
    for n in ["rating_head.0.weight", "rating_head.2.weight", "transformers.norm.scale", "action_embedding.linear.weight"] + \
             [f"transformers.layers.{l}.{t}" for l in (0, 7) for t in ("attn.q_proj.weight", "attn.k_proj.weight", "attn.v_proj.weight",
                                                                        "attn.output_proj.weight", "mlp.w1.weight", "mlp.w2.weight",
                                                                        "mlp.w3.weight", "sa_norm.scale", "mlp_norm.scale")]:
        g = model.grad(n)
        scale = max(np.abs(G_ref[n]).max(), 1e-12)
        assert np.abs(g - G_ref[n]).max() / scale < 1e-3, (n, np.abs(g - G_ref[n]).max() / scale)
    model.close()

    # ---- (2) bf16, 4 rows: isolation and permutation
    rows = 4
    d = synth.make_batch(cfg, rows, 321, mu=4.0, sigma=0.8)
    wm, rm = synth.make_masks(cfg, rows, 9)
    model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=rows)
    model.init_weights(5)
    model.load_pretrained_embeddings(table)
    model.set_loss_weights(TASK_W, 1)
    model(d, True, masks=(wm, rm))
    y0 = model.trunk_output(rows).copy()
    uid = np.asarray(d["userid"]).reshape(rows, S)
    victim = uid[1, S // 2]
    sel = (uid == victim)
    assert sel.any() and not sel.all()
    d2 = {k: np.array(v, copy=True) for k, v in d.items()}
    flat = sel.reshape(-1)
    d2["rating"] = np.where(flat, 10.0 - np.asarray(d["rating"]).reshape(-1), np.asarray(d["rating"]).reshape(-1)).astype(np.float32)
    mid = np.asarray(d["matchedid"]).reshape(-1)
    d2["matchedid"] = np.where(flat, (mid + 17) % V, mid).astype(np.int32)
    model(d2, True, masks=(wm, rm))
    y1 = model.trunk_output(rows)
    tok = np.repeat(sel, 2, axis=1)
    assert np.array_equal(y0[~tok], y1[~tok])
    assert np.abs(y0[tok] - y1[tok]).max() > 1e-3
    perm = np.array([2, 0, 3, 1])
    dp = {k: np.asarray(v).reshape(rows, S)[perm].reshape(-1) for k, v in d.items()}
    model(dp, True, masks=(wm[perm], rm[perm]))
    assert np.array_equal(model.trunk_output(rows), y0[perm])
    model.close()


ODD_SHAPES = [
    # embed_dim, heads, kv heads, intermediate, seq, vocab 0 / 1, metadata, topk, rows
    dict(D=192, H=3, KV=1, I=520, S=40, V0=777, V1=1234, M=37, K=5, rows=3),      # hd 64, 3 query heads per kv head, T = 80
    dict(D=64, H=4, KV=4, I=72, S=24, V0=9, V1=11, M=3, K=3, rows=1),              # hd 16, no GQA sharing, tiny vocabularies
    dict(D=320, H=5, KV=5, I=904, S=136, V0=2049, V1=513, M=129, K=17, rows=2),    # T = 272: 4 full + 1 partial attention tile
    dict(D=128, H=4, KV=2, I=344, S=36, V0=301, V1=222, M=20, K=4, rows=2),        # hd 32
    dict(D=256, H=2, KV=1, I=696, S=68, V0=150, V1=333, M=41, K=7, rows=2),        # hd 128
]


@pytest.mark.parametrize("shape", ODD_SHAPES)
@pytest.mark.parametrize("dtype,tol_loss,tol_act,tol_grad", [("fp32", 1e-4, 1e-4, 5e-4), ("bf16", 4e-2, 6e-2, 1.5e-1)])
def test_irregular_shapes_vs_oracle(shape, dtype, tol_loss, tol_act, tol_grad):
    """Shapes no tile size divides (the reference accepts any configuration with head_dim 16 or 64 here): sequence lengths
    that leave partial attention tiles, intermediate / vocabulary / metadata sizes that leave partial GEMM tiles and odd
    leading dimensions, 1:1 and 3:1 query-to-kv head ratios, a single row."""
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config("tiny", mask_rate=0.2, mask_topk=shape["K"], num_heads=shape["H"], num_kv_heads=shape["KV"],
                            embed_dim=shape["D"], intermediate_dim=shape["I"], max_sequence_length=shape["S"],
                            metadata_emb_size=shape["M"])
    cfg["vocab_sizes"]["0_matchedid"] = shape["V0"]; cfg["vocab_sizes"]["1_matchedid"] = shape["V1"]
    rows, seed = shape["rows"], 61
    P = synth.make_params(cfg, seed, "test")
    d = synth.make_batch(cfg, rows, seed + 1, mu=2.5, sigma=0.9)
    wm, rm = synth.make_masks(cfg, rows, seed + 2)
    y_ref, l_ref, G_ref, ev_ref = _oracle(cfg, P, d, wm, rm)
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
    model.load_state_dict(P)
    model.set_loss_weights(TASK_W, 1)
    losses = model(d, False, masks=(wm, rm))
    assert relerr(model.trunk_output(rows), y_ref) < tol_act
    for a, b in zip(losses, l_ref):
        assert abs(a - b) <= tol_loss * max(abs(b), 1.0), (losses, l_ref)
    worst = ("", 0.0)
    for n in synth.trainable_names(cfg):
        g = model.grad(n)
        scale = max(np.abs(G_ref[n]).max(), 1e-3 * np.sqrt((G_ref[n] ** 2).mean()) + 1e-12)
        e = float(np.abs(g - G_ref[n]).max() / max(scale, 1e-6))
        if e > worst[1]:
            worst = (n, e)
    assert worst[1] < tol_grad, worst
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_inference_select_equals_the_full_forward_and_sees_parameter_changes(dtype):
    """rsys_infer_select reports exactly the rows rsys_infer reports for the same tokens (retrieval: trunk rows; ranking: the
    rating head evaluated on those rows only), and the fused item table cached between inference calls is rebuilt after a
    parameter of it changes."""
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config("hd64")
    rows = 3
    S = cfg["max_sequence_length"]
    P = synth.make_params(cfg, 9, "test")
    d = synth.make_batch(cfg, rows, 10)
    d["rope_input_pos"] = np.tile(np.arange(S, dtype=np.int32), rows)
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
    model.load_state_dict(P)
    full_r = model(d, "retrieval"); full_k = model(d, "ranking")
    rng = np.random.default_rng(3)
    idx = rng.choice(rows * 2 * S, size=37, replace=False).astype(np.int32)
    sel_r = model.inference_select(d, "retrieval", idx)
    sel_k = model.inference_select(d, "ranking", idx)
    assert np.array_equal(sel_r, full_r.reshape(-1, cfg["embed_dim"])[idx])
    assert np.allclose(sel_k, full_k.reshape(-1)[idx], rtol=1e-6, atol=1e-6)
    again = model(d, "retrieval")                      # cached table: same bits
    assert np.array_equal(again, full_r)
    name = "item_embedding.projection_layer.bias"
    model.set_parameter(name, P[name] + np.float32(0.25))
    moved = model(d, "retrieval")
    assert np.abs(moved - full_r).max() > 1e-3          # the table was rebuilt with the new bias
    model.set_parameter(name, P[name])
    assert np.array_equal(model(d, "retrieval"), full_r)
    with pytest.raises(Exception):
        model.inference_select(d, "retrieval", [rows * 2 * S])
    model.close()


@pytest.mark.parametrize("dtype,tol_loss,tol_grad", [("fp32", 1e-4, 5e-4), ("bf16", 4e-2, 1.5e-1)])
def test_partial_batch_and_rows_without_targets(dtype, tol_loss, tol_grad):
    """Ragged inputs through the compact top: a model built for 5 rows fed 3 (the compact buffers, the selected-first order and
    the tile maps are sized for max_rows), one of them with no target at all (its leading query tiles count is zero: the last
    layer's attention skips the row) and one whose masks select a single position.  Losses, dense trunk output and every
    gradient against the oracle."""
    import recommendersystem_amd as ra
    from oracle import synth
    cfg, P, d = _setup("hd64", dict(mask_rate=0.2, mask_topk=16), 3, 61)
    S = cfg["max_sequence_length"]
    wm, rm = synth.make_masks(cfg, 3, 63)
    wm[1] = False; rm[1] = False                      # row 1: nothing masked, so nothing selected
    wm[2] = False; rm[2] = False; wm[2, S // 2] = True   # row 2: one watch position
    y_ref, l_ref, G_ref, _ = _oracle(cfg, P, d, wm, rm)
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=5)
    model.load_state_dict(P)
    model.set_loss_weights(TASK_W, 1)
    losses = model(d, False, masks=(wm, rm))
    assert relerr(model.trunk_output(3), y_ref) < (1e-4 if dtype == "fp32" else 6e-2)
    for a, b in zip(losses, l_ref):
        assert abs(a - b) <= tol_loss * max(abs(b), 1.0), (losses, l_ref)
    for n in synth.trainable_names(cfg):
        assert np.abs(model.grad(n) - G_ref[n]).max() <= tol_grad * max(np.abs(G_ref[n]).max(), 1e-9), n
    if int(model.debug_get("top.cap", 3)[0]) > 0:
        slot = model.debug_get("top.slot", 3).reshape(3, 2 * S)
        assert (slot[1] == -1).all() and (slot[2] >= 0).sum() <= 1
    model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_batch_without_any_target_gives_zero_losses_and_gradients(dtype):
    """Every target weight zero (a shard tail of padding): nothing is selected, the compact row set is empty, the step must
    produce zero losses and all-zero finite gradients -- not NaNs from empty reductions."""
    import recommendersystem_amd as ra
    from oracle import synth
    cfg, P, d = _setup("hd64", dict(mask_rate=0.2, mask_topk=16), 2, 71)
    d = {k: (np.zeros_like(v) if k.endswith(".weight") else v) for k, v in d.items()}
    wm, rm = synth.make_masks(cfg, 2, 73)
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=2)
    model.load_state_dict(P)
    model.set_loss_weights(TASK_W, 1)
    losses = model(d, False, masks=(wm, rm))
    assert all(abs(x) == 0.0 for x in losses), losses
    if int(model.debug_get("top.cap", 2)[0]) > 0:
        assert int(model.debug_get("top.n", 2)[0]) == 0
    for n in synth.trainable_names(cfg):
        g = model.grad(n)
        assert np.isfinite(g).all() and np.abs(g).max() == 0.0, n
    assert np.isfinite(model.trunk_output(2)).all()
    model.close()


def test_call_site_timer_gives_up_quietly_when_nobody_collects():
    """`model.timing(True)` takes two HIP events per kernel call site and step.  A caller that never collects the report runs the pool
    to its bound (8192 events); the timer must then switch itself off and the steps must go on -- an unchecked event record used to
    surface as `invalid resource handle` at the next launch check (bench.py --detail at the production shape, round 4) -- and a
    collected report must still carry whole (begin, end) pairs only."""
    import recommendersystem_amd as ra
    from oracle import synth
    name, over, rows, seed = CASES[1]
    cfg, P, d = _setup(name, over, rows, seed)
    wm, rm = synth.make_masks(cfg, rows, 5)
    model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=rows)
    model.load_state_dict(P)
    model.set_loss_weights(TASK_W, 1)
    model.timing(True, serialize=True)
    first = None
    for i in range(120):                      # a few hundred events per step: the bound is passed well before the end
        losses = model(d, False, masks=(wm, rm))
        assert np.all(np.isfinite(losses))
        if first is None:
            first = np.array(losses)
    rep = model.timing_report()
    assert rep and all(v["count"] >= 1 and v["ms"] >= 0.0 for v in rep.values())
    per_step = max(v["count"] for k, v in rep.items() if k.startswith("phase_trunk_fwd"))
    assert 1 <= per_step < 120                # it stopped measuring before the last step ...
    model.timing(True)                        # ... and can be switched on again
    model(d, False, masks=(wm, rm))
    rep2 = model.timing_report()
    assert rep2["phase_trunk_fwd"]["count"] == 1
    model.timing(False)
    model.close()


def test_call_site_timer_filter_and_pause():
    """bench.py times only the dominant kernel family's call sites inside its timed region (`timing_filter`: sites whose name contains
    the substring; nested phase spans that do not match record nothing) and reads them after the region (`timing_pause`: recording stops
    without a host wait, what was recorded stays readable).  Same losses with and without the timer."""
    import recommendersystem_amd as ra
    from oracle import synth
    name, over, rows, seed = CASES[1]
    cfg, P, d = _setup(name, over, rows, seed)
    wm, rm = synth.make_masks(cfg, rows, 5)
    model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=rows)
    model.load_state_dict(P)
    model.set_loss_weights(TASK_W, 1)
    plain = np.array(model(d, False, masks=(wm, rm)))
    model.zero_grad()
    model.timing(True)
    full = None
    np.testing.assert_allclose(np.array(model(d, False, masks=(wm, rm))), plain, rtol=1e-6)   # (loss sums use float atomics)
    full = model.timing_report()
    model.zero_grad()
    assert any(k.startswith("phase_") for k in full) and any(k.startswith("gemm_") for k in full)
    fam = sorted({k.split("@")[1] for k in full if k.startswith("gemm_") and "@" in k})[0]
    model.timing_filter("@" + fam)
    model(d, False, masks=(wm, rm)); model.zero_grad()
    model(d, False, masks=(wm, rm)); model.zero_grad()
    model.timing_pause()
    model(d, False, masks=(wm, rm)); model.zero_grad()          # not recorded
    rep = model.timing_report()
    assert rep and all(k.endswith("@" + fam) for k in rep), sorted(rep)
    for k, v in rep.items():
        assert v["count"] == 2 * full[k]["count"], (k, v, full[k])
    model.timing(False)                                          # clears the filter
    model.timing(True)
    model(d, False, masks=(wm, rm))
    assert any(k.startswith("phase_") for k in model.timing_report())
    model.timing(False)
    model.close()
