"""GPU: the call sites of one training step, as the call-site timer reports them (`model.timing(True, serialize=True)`): which tags
appear, how often, and with how many flops (GEMMs) or bytes (hbm_*).  The expected values are computed here from the configuration
alone, for every route the step's host code takes: compact or dense top, grouped or per-layer weight gradients, fp32, the fp8 trunk,
the LoRA finetune with dropout, and an evaluation pass.  bench.py corrects flops by tag name, so a renamed, missing or extra
`gemm_*` / `attn_*` / `hbm_*` / `phase_*` tag fails here.

The report prints a tag's flops with six significant digits, so the sums are compared to 1e-5 of their value; counts are exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TASK_W = [0.05, 0.2, 0.3, 0.25]
FAMILIES = ("gemm_", "attn_", "hbm_", "phase_")

ARMS = {
    # id: (config, rows, dtype, environment, config overrides, evaluate)
    "bf16": ("hd64", 4, "bf16", {}, {}, False),
    "bf16-cfg1": ("cfg1", 16, "bf16", {}, {}, False),
    "dense-top": ("hd64", 4, "bf16", {"RSYS_SPARSE_TOP": "0"}, {}, False),
    "per-layer-dw": ("hd64", 4, "bf16", {"RSYS_DW_GROUP": "0"}, {}, False),
    "fp32": ("hd64", 4, "fp32", {}, {}, False),
    "fp8": ("f8t", 4, "fp8", {}, {"mask_topk": 16}, False),          # (the smallest shape the fp8 trunk takes)
    "lora-dropout": ("hd64", 4, "bf16", {}, {"finetune": True, "finetune_metric": "rating", "lora_dropout": 0.1}, False),
    "evaluate": ("hd64", 4, "bf16", {}, {}, True),
}


def _pad(n, q):
    return (n + q - 1) // q * q


def expected_call_sites(cfg, rows, dtype, compact, grouped, evaluate, cap):
    """tag -> (count, summed flops or bytes) of one step (forward, backward, optimizer step) of a replicated-table model"""
    L, D, I, S = cfg["num_layers"], cfg["embed_dim"], cfg["intermediate_dim"], cfg["max_sequence_length"]
    H, KV = cfg["num_heads"], cfg["num_kv_heads"]
    hd = D // H
    V0, V1 = cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"]
    fp8, ft = dtype == "fp8", bool(cfg.get("finetune"))
    esz, cp = (4, 0) if dtype == "fp32" else (2, 2)          # bytes of the compute type; of the gradient's operand copy
    Ip = _pad(I, 128 if fp8 else 16)
    Nqkv = (H + 2 * KV) * hd
    N = rows * S
    NT, KB = 2 * N, cfg["mask_topk"] * rows
    TR, Mp = V0 + V1 + 1, _pad(cfg["metadata_emb_size"], 64)
    train = not evaluate
    dense_layers = L - 1 if compact else L                   # layers whose token-local tail runs on all NT tokens
    qkv, o, w13, w2 = 2.0 * NT * Nqkv * D, 2.0 * NT * D * D, 2.0 * NT * 2 * Ip * D, 2.0 * NT * D * Ip
    top = {"o": 2.0 * cap * D * D, "w13": 2.0 * cap * 2 * Ip * D, "w2": 2.0 * cap * D * Ip}
    e = {}

    def add(tag, count, each):
        if count:
            e[tag] = (count, count * each)

    # forward
    for tag in ("phase_embed", "phase_trunk_fwd", "phase_heads"):
        add(tag, 1, 0.0)
    add("gemm_table_fwd", 1, 2.0 * TR * D * Mp)
    add("gemm_action_fwd", 1, 2.0 * N * D * 32)
    add("hbm_gather", 1, 8.0 * D * N)
    add("hbm_rmsnorm_fwd", L + dense_layers + (0 if compact else 1), (4.0 + esz) * D * NT)
    add("gemm_qkv_fwd", L, qkv)
    add("attn_fwd", L, 0.0)
    for name, fl in (("o", o), ("w13", w13), ("w2", w2)):
        add(f"gemm_{name}_fwd", dense_layers, fl)
        if compact:
            add(f"gemm_top_{name}_fwd", 1, top[name])
    if compact:
        add("phase_top_compact_fwd", 1, 0.0)
    if ft:
        add("gemm_lora_a_fwd", L, 2.0 * NT * 16 * D)
        add("gemm_lora_b_fwd", L, 2.0 * NT * Nqkv * 16)
    add("gemm_logits", 2, 2.0 * KB * D * (V0 + V1) / 2)
    add("gemm_rating_fwd", 2, 2.0 * KB * D * D)
    if fp8:   # a training pass: eight products per layer, each with a cast that reads its operand and writes it and its transposed copy
        assert train
        e["hbm_f8_cast"] = (8 * L, 4.0 * NT * (5 * D + Ip + 2 * Ip + Nqkv) * L)
    if evaluate:
        return e
    # backward
    add("phase_trunk_bwd", 1, 0.0)
    add("gemm_head_dx", 2, 2.0 * KB * D * (V0 + V1) / 2)
    add("gemm_rating_dx", 2, 2.0 * KB * D * D)
    nb = (esz + 12.0 + cp) * D * NT
    n_norm = L + dense_layers
    e["hbm_rmsnorm_bwd"] = (n_norm + (0 if compact else 1), n_norm * nb + (0 if compact else (12.0 + cp) * D * NT))
    add("attn_bwd", L, 0.0)
    add("gemm_qkv_dx", L, qkv)
    for name, fl in (("o", o), ("w13", w13), ("w2", w2)):
        add(f"gemm_{name}_dx", dense_layers, fl)
        if compact:
            add(f"gemm_top_{name}_dx", 1, top[name])
            if not ft:
                add(f"gemm_top_{name}_dw", 1, top[name])
    if compact:
        add("phase_top_compact_bwd", 1, 0.0)
    if ft:
        add("gemm_lora_dla", L, 2.0 * NT * 16 * Nqkv)
        add("gemm_lora_db", 2 * L, 2.0 * NT * 8 * (H + KV) * hd / 2)
        add("gemm_lora_da", L, 2.0 * NT * 16 * D)
        add("gemm_lora_dx", L, 2.0 * NT * D * 16)
        return e                                              # the base weights, the embeddings and the table are frozen
    if grouped:
        add("gemm_dw_group", 1, L * qkv + dense_layers * (o + w13 + w2))
    else:
        add("gemm_qkv_dw", L, qkv)
        for name, fl in (("o", o), ("w13", w13), ("w2", w2)):
            add(f"gemm_{name}_dw", dense_layers, fl)
    add("gemm_head_dw", 2, 2.0 * KB * D * (V0 + V1) / 2)
    add("gemm_rating_dw", 2, 2.0 * KB * D * D)
    add("phase_embed_bwd", 1, 0.0)
    add("hbm_scatter", 1, 12.0 * D * N)
    add("gemm_action_dw", 1, 2.0 * N * D * 32)
    add("gemm_action_dx", 1, 2.0 * N * D * 32)
    # optimizer step: dWp from the accumulated table gradient (bf16: over the table rows padded to the K tile)
    add("phase_table_bwd", 1, 0.0)
    add("gemm_table_dw", 1, 2.0 * D * Mp * (TR if dtype == "fp32" else _pad(TR, 64)))
    return e


@pytest.fixture
def switches(monkeypatch):
    """set(env): the environment for the models the test creates, switches re-parsed; both restored afterwards"""
    from recommendersystem_amd._lib import lib

    def set_env(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        lib().rsys_switches_reload()
    yield set_env
    monkeypatch.undo()
    lib().rsys_switches_reload()


@pytest.mark.parametrize("arm", list(ARMS))
def test_call_sites_of_one_step(arm, switches):
    import recommendersystem_amd as ra
    from oracle import synth
    name, rows, dtype, env, over, evaluate = ARMS[arm]
    switches(env)
    cfg = synth.make_config(name, mask_rate=0.2, **over)
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
    try:
        model.load_state_dict(synth.make_params(cfg, 3, "test"), strict=not cfg.get("finetune"))
        opt = ra.create_optimizer(model, dict(cfg, learning_rate=1e-2))
        model.set_loss_weights(TASK_W, 1)
        d, mk = synth.make_batch(cfg, rows, 40), synth.make_masks(cfg, rows, 50)
        model.timing(True, serialize=True)
        losses = model(d, evaluate, masks=mk)
        if not evaluate:
            opt.step(clip_max_norm=1.0)
        rep = model.timing_report()
        model.timing(False)
        cap = int(model.debug_get("top.cap", rows)[0])
    finally:
        model.close()
    assert np.isfinite(np.array([x for l in losses for x in (l if isinstance(l, list) else [l])])).all()
    compact = env.get("RSYS_SPARSE_TOP") != "0" and dtype != "fp8" and not evaluate
    grouped = env.get("RSYS_DW_GROUP") != "0" and dtype != "fp32" and not cfg.get("finetune")
    assert (cap > 0) == compact, (cap, compact)
    got = {}
    for full, v in rep.items():
        tag = full.split("@")[0]
        if tag.startswith(FAMILIES):
            c, f = got.get(tag, (0, 0.0))
            got[tag] = (c + v["count"], f + v["flops"])
    want = expected_call_sites(cfg, rows, dtype, compact, grouped, evaluate, cap)
    print(arm, "cap", cap, {k: got[k] for k in sorted(got)})
    assert sorted(got) == sorted(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    for tag, (count, flops) in want.items():
        assert got[tag][0] == count, (tag, got[tag], count)
        assert abs(got[tag][1] - flops) <= 1e-5 * flops, (tag, got[tag], flops)
