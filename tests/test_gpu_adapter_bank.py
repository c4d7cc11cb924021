"""GPU: the adapter bank (rsys_adapter_*, rsys_infer_select_adapters) -- several LoRA adapters on one base model, one
slot per batch row -- against the fp64 oracle run per adapter, against the existing single-adapter path (a finetune = 1 model with
the same tensors), and its exact properties (row independence, determinism, storage round trip, no side effect on the model)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _adapter_bank_util as ab  # noqa: E402

pytestmark = pytest.mark.gpu

CONFIGS = [("tiny", dict(mask_rate=0.25, mask_topk=6), 6), ("hd64", dict(mask_rate=0.2, mask_topk=16), 6)]
SLOTS = [0, 1, 2, 3, -1, 2]
TASK_W = [0.05, 0.2, 0.3, 0.25]


def relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _setup(name, over, rows, seed=21):
    from oracle import synth
    cfg = synth.make_config(name, **over)
    cfg["forward"] = "inference"
    S = cfg["max_sequence_length"]
    P = synth.make_params(cfg, seed, "test")
    d = synth.make_batch(cfg, rows, seed + 1)
    d["rope_input_pos"] = np.tile(np.arange(S, dtype=np.int32), rows)
    adapters = ab.make_adapters(cfg, 4, seed + 50)
    rng = np.random.default_rng(seed + 2)
    per_row = min(9, 2 * S)
    idx = np.concatenate([r * 2 * S + np.sort(rng.choice(2 * S, size=per_row, replace=False)) for r in range(rows)]).astype(np.int32)
    return cfg, P, d, adapters, idx, per_row


def _bank_model(cfg, P, adapters, dtype, rows):
    import recommendersystem_amd as ra
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
    model.load_state_dict(P)
    for s, ad in enumerate(adapters):
        model.load_adapter(s, ad)
    return model


def _rows_of(vals, per_row, rows):
    return np.asarray(vals).reshape(rows, per_row, -1)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name,over,rows", CONFIGS)
def test_bank_rows_against_the_oracle_and_the_single_adapter_path(name, over, rows, dtype):
    """Adapters: oracle.synth "test" style, A ~ N(0, 1 / D), B ~ N(0, 1 / 8): the update has about twice the projection's standard
    deviation.  Per row: selected outputs against OracleModel(finetune cfg, base + the row's adapter).inference in float64 (slot -1:
    the base oracle).  fp32: relative error < 1e-4.  bf16: the bank's error must not exceed 1.5 x the error of the existing path (a
    finetune = 1 model holding the same tensors, rsys_infer_select) measured on the same rows against the same oracle."""
    import recommendersystem_amd as ra
    from oracle import model_np
    cfg, P, d, adapters, idx, per_row = _setup(name, over, rows)
    ft_cfg = ab.finetune_config(cfg)
    slots = SLOTS[:rows]
    d2 = model_np.reshape_batch(cfg, d)
    bank = _bank_model(cfg, P, adapters, dtype, rows)
    ft = ra.RecommenderModel(ft_cfg, dtype=dtype, max_rows=rows)
    ft.load_state_dict(dict(P, **adapters[0]))
    for task in ("retrieval", "ranking"):
        got = _rows_of(bank.inference_select(d, task, idx, adapters=slots), per_row, rows)
        base_dev = _rows_of(bank.inference_select(d, task, idx), per_row, rows)
        ref = np.empty(got.shape, np.float64)
        old = np.empty(got.shape, np.float64)
        for s in sorted(set(slots)):
            mine = [r for r in range(rows) if slots[r] == s]
            if s < 0:
                full = model_np.OracleModel(cfg, P, np.float64).inference(d2, task)
                dev = base_dev
            else:
                full = model_np.OracleModel(ft_cfg, dict(P, **adapters[s]), np.float64).inference(d2, task)
                for k, v in adapters[s].items():
                    ft.set_parameter(k, v)
                dev = _rows_of(ft.inference_select(d, task, idx), per_row, rows)
            flat = np.asarray(full).reshape(rows * 2 * cfg["max_sequence_length"], -1)[idx].reshape(got.shape)
            ref[mine] = flat[mine]; old[mine] = dev[mine]
        e_bank = [relerr(got[r], ref[r]) for r in range(rows)]
        e_old = [relerr(old[r], ref[r]) for r in range(rows)]
        with_ad = [r for r in range(rows) if slots[r] >= 0]
        eb, eo = relerr(got[with_ad], ref[with_ad]), relerr(old[with_ad], ref[with_ad])
        moved = min(relerr(got[r], base_dev[r]) for r in with_ad)
        print(f"adapter bank {name} {dtype} {task}: bank err {eb:.3e} (rows {['%.2e' % x for x in e_bank]}), single-adapter path err {eo:.3e} "
              f"(rows {['%.2e' % x for x in e_old]}), least distance from the base model {moved:.3e}")
        if dtype == "fp32":
            assert max(e_bank) < 1e-4, (task, e_bank)
        else:
            assert eb <= 1.5 * eo, (task, eb, eo)
        # not a no-op: with an adapter the outputs are far from the base model's, far beyond the tolerance
        assert moved > (1e-2 if dtype == "fp32" else 10 * max(eo, 1e-3)), (task, moved)
        none_rows = [r for r in range(rows) if slots[r] < 0]
        assert np.array_equal(got[none_rows], base_dev[none_rows])
    bank.close(); ft.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bank_exact_properties(dtype):
    name, over, rows = CONFIGS[1]
    cfg, P, d, adapters, idx, per_row = _setup(name, over, rows, seed=33)
    bank = _bank_model(cfg, P, adapters, dtype, rows)
    for task in ("retrieval", "ranking"):
        run = lambda slots: _rows_of(bank.inference_select(d, task, idx, adapters=slots), per_row, rows)
        # all rows -1: the base model's call, byte for byte
        assert np.array_equal(run([-1] * rows), _rows_of(bank.inference_select(d, task, idx), per_row, rows))
        # row independence: row 2 with slot 1, whatever the others do
        a = run([1] * rows); b = run([0, 3, 1, 2, -1, 0]); c = run([-1, -1, 1, -1, -1, -1])
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[2], c[2])
        assert not np.array_equal(a[0], b[0])
        # two identical calls
        assert np.array_equal(run(SLOTS), run(SLOTS))
        # a scalar means every row
        assert np.array_equal(a, _rows_of(bank.inference_select(d, task, idx, adapters=1), per_row, rows))
    # the same adapter in two slots gives the same rows
    bank.load_adapter(5, adapters[2])
    assert bank.adapters_loaded() == [0, 1, 2, 3, 5]
    x = _rows_of(bank.inference_select(d, "retrieval", idx, adapters=[2] * rows), per_row, rows)
    y = _rows_of(bank.inference_select(d, "retrieval", idx, adapters=[5] * rows), per_row, rows)
    assert np.array_equal(x, y)
    # storage round trip, bit for bit
    for s, ad in [(0, adapters[0]), (3, adapters[3]), (5, adapters[2])]:
        sd = bank.adapter_state_dict(s)
        assert sorted(sd) == sorted(ad) and all(sd[k].dtype == np.float32 and np.array_equal(sd[k], ad[k]) for k in ad)
    # clearing a slot: rows naming it are refused, the others' results do not move
    before = _rows_of(bank.inference_select(d, "ranking", idx, adapters=[0, 1, 3, 3, -1, 0]), per_row, rows)
    bank.clear_adapter(2)
    assert bank.adapters_loaded() == [0, 1, 3, 5]
    import recommendersystem_amd as ra
    with pytest.raises(ra.RsysError):
        bank.inference_select(d, "ranking", idx, adapters=[0, 1, 2, 3, -1, 0])
    assert np.array_equal(before, _rows_of(bank.inference_select(d, "ranking", idx, adapters=[0, 1, 3, 3, -1, 0]), per_row, rows))
    bank.load_adapter(2, adapters[2])                              # a cleared slot can be filled again
    assert np.array_equal(x, _rows_of(bank.inference_select(d, "retrieval", idx, adapters=[2] * rows), per_row, rows))
    bank.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bank_leaves_the_model_untouched(dtype):
    """Loading / clearing slots and running the bank forward change nothing else: state_dict, item table, a retrieve_topk result, and
    the losses and gradients of a following training step (deterministic mode) are byte-equal to a model that never had a bank."""
    import recommendersystem_amd as ra
    from oracle import synth
    name, over, rows = CONFIGS[1]
    cfg, P, d, adapters, idx, per_row = _setup(name, over, rows, seed=44)
    cfg = dict(cfg, forward="train")
    wm, rm = synth.make_masks(cfg, rows, 7)
    dt = {k: v for k, v in d.items() if k != "rope_input_pos"}
    grads = ["transformers.layers.0.attn.q_proj.weight", "transformers.layers.1.mlp.w2.weight", "item_embedding.projection_layer.weight",
             "item_embedding.matchedid_embedding.embedding.weight", "rating_head.0.weight"]

    def observe(with_bank):
        m = ra.RecommenderModel(cfg, dtype=dtype, max_rows=rows)
        m.set_deterministic(True)
        m.load_state_dict(P)
        table0 = m.item_embeddings()
        q = m.inference_select(d, "retrieval", idx)[:4]
        top0 = m.retrieve_topk(q, 1, 5)
        if with_bank:
            for s, ad in enumerate(adapters):
                m.load_adapter(s, ad)
            m.inference_select(d, "retrieval", idx, adapters=SLOTS[:rows])
            m.clear_adapter(1)
        sd = m.state_dict()
        table = m.item_embeddings()
        top = m.retrieve_topk(q, 1, 5)
        assert np.array_equal(table, table0) and all(np.array_equal(a, b) for a, b in zip(top, top0))
        m.set_loss_weights(TASK_W)
        m.zero_grad()
        losses = m(dt, False, masks=(wm, rm))
        g = {k: m.grad(k) for k in grads}
        m.close()
        return sd, table, top, losses, g

    a, b = observe(False), observe(True)
    assert sorted(a[0]) == sorted(b[0]) and all(np.array_equal(a[0][k], b[0][k]) for k in a[0])
    assert not any("lora_" in k for k in b[0])
    assert np.array_equal(a[1], b[1])
    assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
    assert a[3] == b[3], (a[3], b[3])
    assert all(np.array_equal(a[4][k], b[4][k]) for k in grads)


def test_bank_argument_errors_leave_the_output_unwritten():
    import ctypes as C

    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd._lib import lib
    cfg, P, d, adapters, idx, per_row = _setup("tiny", CONFIGS[0][1], 2)
    D, L = cfg["embed_dim"], cfg["num_layers"]
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=2)
    model.load_state_dict(P)
    Lb, h = lib(), model._h
    qa = "transformers.layers.0.attn.q_proj_lora_A.weight".encode()
    good = np.ascontiguousarray(adapters[0][qa.decode()])
    SENT = np.float32(-7.25)
    buf = np.full(8 * D, SENT, np.float32)
    ARG = -1
    assert Lb.rsys_adapter_set(h, 8, qa, good.ctypes.data, good.size) == ARG
    assert Lb.rsys_adapter_set(h, -1, qa, good.ctypes.data, good.size) == ARG
    assert Lb.rsys_adapter_set(h, 0, b"transformers.layers.0.attn.k_proj_lora_A.weight", good.ctypes.data, good.size) == ARG
    assert Lb.rsys_adapter_set(h, 0, f"transformers.layers.{L}.attn.q_proj_lora_A.weight".encode(), good.ctypes.data, good.size) == ARG
    assert Lb.rsys_adapter_set(h, 0, qa, good.ctypes.data, good.size - 1) == ARG
    assert Lb.rsys_adapter_get(h, 0, qa, buf.ctypes.data, buf.size) == ARG and (buf == SENT).all()      # not set yet
    mask = C.c_int32(-1)
    assert Lb.rsys_adapter_slots(h, C.byref(mask)) == 0 and mask.value == 0
    assert Lb.rsys_adapter_set(h, 0, qa, good.ctypes.data, good.size) == 0
    assert Lb.rsys_adapter_get(h, 0, qa, buf.ctypes.data, buf.size - 1) == ARG and (buf == SENT).all()
    assert Lb.rsys_adapter_get(h, 9, qa, buf.ctypes.data, buf.size) == ARG and (buf == SENT).all()
    assert Lb.rsys_adapter_slots(h, C.byref(mask)) == 0 and mask.value == 0                               # 1 of 4 L tensors: incomplete
    with pytest.raises(KeyError):
        model.load_adapter(1, {k: v for k, v in adapters[1].items() if "layers.1.attn.v_proj_lora_B" not in k})
    assert model.adapters_loaded() == []
    model.load_adapter(1, adapters[1])
    assert model.adapters_loaded() == [1]
    out = np.full(idx.size * D, SENT, np.float32)
    rows_ok = np.array([1, -1], np.int32)
    call = lambda task, rows, index, n_idx, n_out: Lb.rsys_infer_select_adapters(
        h, task, None if rows is None else rows.ctypes.data, index.ctypes.data, n_idx, out.ctypes.data, n_out)
    assert call(0, rows_ok, idx, idx.size, out.size) == ARG and (out == SENT).all()                       # no batch uploaded
    model.upload(d)
    assert call(0, None, idx, idx.size, out.size) == ARG and (out == SENT).all()                          # row_adapter NULL
    assert call(0, np.array([1, 0], np.int32), idx, idx.size, out.size) == ARG and (out == SENT).all()   # slot 0 is incomplete
    assert call(0, np.array([1, 8], np.int32), idx, idx.size, out.size) == ARG and (out == SENT).all()
    assert call(0, np.array([-2, 1], np.int32), idx, idx.size, out.size) == ARG and (out == SENT).all()
    assert call(2, rows_ok, idx, idx.size, out.size) == ARG and (out == SENT).all()
    assert call(0, rows_ok, idx, idx.size, out.size - 1) == ARG and (out == SENT).all()
    bad_idx = idx.copy(); bad_idx[0] = 2 * 2 * cfg["max_sequence_length"]
    assert call(0, rows_ok, bad_idx, idx.size, out.size) == ARG and (out == SENT).all()
    assert call(0, rows_ok, idx, idx.size, out.size) == 0 and not (out == SENT).any()
    model.close()
    # a finetune = 1 model owns its adapter; an fp8 model has none
    ft = ra.RecommenderModel(ab.finetune_config(cfg), dtype="fp32", max_rows=2)
    assert Lb.rsys_adapter_set(ft._h, 0, qa, good.ctypes.data, good.size) == ARG
    assert Lb.rsys_adapter_clear(ft._h, 0) == ARG and Lb.rsys_adapter_slots(ft._h, C.byref(mask)) == ARG
    ft.upload(d)
    assert Lb.rsys_infer_select_adapters(ft._h, 0, rows_ok.ctypes.data, idx.ctypes.data, idx.size, out.ctypes.data, out.size) == ARG
    ft.close()
    cfg8 = synth.make_config("f8t")
    m8 = ra.RecommenderModel(cfg8, dtype="fp8", max_rows=1)
    a8 = np.zeros(8 * cfg8["embed_dim"], np.float32)
    assert Lb.rsys_adapter_set(m8._h, 0, qa, a8.ctypes.data, a8.size) == ARG
    m8.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dedup_get_models_predict_end_to_end(dtype, tmp_path):
    """dedup four tiny finetune checkpoints -> get_models -> predict for the four (medium, task) pairs and predict_mixed over users of
    both media, against predict on four separately built finetune = 1 models (fp32: 1e-4 against the fp64 oracle for both; bf16: the
    bank's error at most 1.5 x the separate models'), and predict_mixed byte-equal to predict row by row."""
    import recommendersystem_amd as ra
    from oracle import model_np, synth
    from recommendersystem_amd import checkpoint, serve
    cfg = synth.make_config("tiny", mask_rate=0.25, mask_topk=6)
    S = cfg["max_sequence_length"]
    n0 = cfg["vocab_sizes"]["0_matchedid"]
    P = synth.make_params(cfg, 31, "test")
    adapters = ab.make_adapters(cfg, 4, 77)
    ft_cfg = ab.finetune_config(cfg)
    paths = []
    for (m, metric), blob in zip(ab.ORDER, ab.finetune_blobs(cfg, P, adapters)):
        paths.append(str(tmp_path / f"{m}.{metric}.npz"))
        np.savez(paths[-1], **blob)
    files = checkpoint.dedup_files(str(tmp_path / "out"), paths)
    load = lambda p: (lambda z: {k: z[k] for k in z.files})(np.load(p))
    model = serve.get_models(load(files[0]), [load(p) for p in files[1:]], ft_cfg, dtype=dtype, max_rows=4)
    assert model.adapter_slots == ab.SLOT_MAP and model.adapters_loaded() == [0, 1, 2, 3]
    rng = np.random.default_rng(9)
    users = [ab.make_user(rng, 5, [3, 7, 11]), ab.make_user(rng, S, [4, 9]), ab.make_user(rng, 3, [2, 5, 6, 8])]
    for task, metric in (("retrieval", "watch"), ("ranking", "rating")):
        mul, mri = (S, 0) if task == "retrieval" else (S // 2, S - S // 2)
        per_pair = {}
        for medium in (0, 1):
            key = f"{medium}.{task}"
            ad = adapters[ab.ORDER.index((medium, metric))]
            got = serve.predict(model, users, task, medium)
            solo = ra.RecommenderModel(dict(ft_cfg, forward="inference"), dtype=dtype, max_rows=4)
            solo.load_state_dict(dict(P, **ad))
            old = serve.predict(solo, users, task, medium)
            solo.close()
            d = serve.build_batch(users, task, medium, n0, mul, mri)
            ref = model_np.OracleModel(ft_cfg, dict(P, **ad), np.float64)
            exp = serve.extract(ref.inference({k: np.asarray(v) for k, v in d.items()}, task), users, task, medium, mul)
            cat = lambda res: np.concatenate([np.asarray(r[key], np.float64).reshape(-1) for r in res])
            eb, eo = relerr(cat(got), cat(exp)), relerr(cat(old), cat(exp))
            print(f"adapter bank end to end {dtype} {key}: bank err {eb:.3e}, separate finetune model err {eo:.3e}")
            if dtype == "fp32":
                assert eb < 1e-4 and eo < 1e-4, (key, eb, eo)
            else:
                assert eb <= 1.5 * eo, (key, eb, eo)
            per_pair[medium] = got
        # users of both media in one forward: same batch shape (3 rows) as the predict calls above -> the same bytes row by row
        media = [1, 0, 1]
        mixed = serve.predict_mixed(model, list(zip(users, media)), task)
        for i, m in enumerate(media):
            key = f"{m}.{task}"
            assert list(mixed[i]) == [key]
            assert np.array_equal(np.asarray(mixed[i][key], np.float32), np.asarray(per_pair[m][i][key], np.float32)), (task, i)
    model.close()
