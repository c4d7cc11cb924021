"""Deterministic mode (rsys_model_set_deterministic): split-K partial tiles summed in split order, reductions through per-workgroup
partials instead of float atomics.  A training step is then bitwise reproducible; the default mode is only reproducible to
float-atomic noise (which these tests also show, so that they cannot pass vacuously)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TASK_W = [0.05, 0.2, 0.3, 0.25]


def _three_steps(cfg, P, batches, masks, dtype, deterministic, fused=True, finetune_P=None):
    import recommendersystem_amd as ra
    from oracle import synth
    rows = len(masks[0][0])
    model = ra.RecommenderModel(dict(cfg, deterministic=deterministic), dtype=dtype, max_rows=rows)
    model.load_state_dict(P, strict=not cfg.get("finetune"))
    opt = ra.create_optimizer(model, dict(cfg, learning_rate=1e-2))
    model.set_loss_weights(TASK_W, 1)
    out = []
    names = synth.trainable_names(cfg)
    for d, mk in zip(batches, masks):
        losses = model(d, False, masks=mk)
        grads = {n: model.grad(n).copy() for n in names}
        if fused:
            opt.step(clip_max_norm=1.0)
        else:
            from recommendersystem_amd.optim import clip_grad_norm_
            clip_grad_norm_(model, 1.0)
            opt.step()
        out.append((np.array(losses, np.float32), grads))
    params = {n: model.get_parameter(n).copy() for n in names}
    model.close()
    return out, params


def _bitwise(a, b):
    (sa, pa), (sb, pb) = a, b
    same = all(np.array_equal(la, lb) and all(np.array_equal(ga[n], gb[n]) for n in ga) for (la, ga), (lb, gb) in zip(sa, sb))
    return same and all(np.array_equal(pa[n], pb[n]) for n in pa)


@pytest.mark.parametrize("name,rows,dtype", [("hd64", 4, "bf16"), ("hd64", 4, "fp32"), ("cfg1", 16, "bf16")])
def test_three_training_steps_are_bitwise_reproducible(name, rows, dtype):
    from oracle import synth
    cfg = synth.make_config(name, mask_rate=0.2)
    P = synth.make_params(cfg, 3, "test")
    batches = [synth.make_batch(cfg, rows, 40 + i) for i in range(3)]
    masks = [synth.make_masks(cfg, rows, 50 + i) for i in range(3)]
    a = _three_steps(cfg, P, batches, masks, dtype, True)
    b = _three_steps(cfg, P, batches, masks, dtype, True)
    assert _bitwise(a, b)
    # and it is the same arithmetic as the default mode, up to the order of the float sums
    c = _three_steps(cfg, P, batches, masks, dtype, False)
    for (la, ga), (lc, gc) in zip(a[0], c[0]):
        assert np.allclose(la, lc, rtol=2e-3 if dtype == "bf16" else 1e-5)
    # the first step's gradients (same parameters in both runs; after it the runs' parameters differ, bounded below): fp32 within
    # the losses' 1e-5 of each tensor's maximum; bf16 within one bf16 ulp (2^-8) of it -- the summation order can flip the rounding of
    # a bf16 operand copy (dx_t, the GEMM operands), which moves the products it enters by at most that much of their magnitude
    ga, gc = a[0][0][1], c[0][0][1]
    for n in ga:
        scale = max(float(np.abs(gc[n]).max()), 1e-30)
        err = float(np.abs(ga[n] - gc[n]).max()) / scale
        assert err <= (2.0 ** -8 if dtype == "bf16" else 1e-5), (n, err)
    # parameters after three Adam steps at lr 1e-2: an element whose gradient is within the summation-order noise of zero may step the other
    # way (+-lr per step), so two runs -- also two runs of the default mode -- may sit up to 2 * 3 * lr apart in such elements; everything
    # else agrees to rounding.  (The former bound, 5e-2 of the tensor's maximum, was that same 6e-2 seen through tensors whose maximum is
    # about one, and a run landed at 0.0505.)
    worst_abs = max(float(np.abs(a[1][n] - c[1][n]).max()) for n in a[1])
    assert worst_abs <= (2.2 * 3 * 1e-2 if dtype == "bf16" else 2e-3), worst_abs
    flipped = max(float((np.abs(a[1][n] - c[1][n]) > 0.5e-2).mean()) for n in a[1] if a[1][n].size >= 1000)
    assert flipped <= (0.05 if dtype == "bf16" else 0.0), flipped      # ... and only a few elements of a tensor do that


def test_default_mode_is_not_bitwise_reproducible_at_this_size():
    """(what the mode is for: with float atomics two runs of the same steps differ in the last bits)"""
    from oracle import synth
    cfg = synth.make_config("cfg1", mask_rate=0.2)
    rows = 32
    P = synth.make_params(cfg, 3, "test")
    batches = [synth.make_batch(cfg, rows, 40 + i) for i in range(3)]
    masks = [synth.make_masks(cfg, rows, 50 + i) for i in range(3)]
    runs = [_three_steps(cfg, P, batches, masks, "bf16", False) for _ in range(3)]
    if _bitwise(runs[0], runs[1]) and _bitwise(runs[0], runs[2]):
        pytest.skip("float atomics happened to land in the same order three times")


def test_fused_clip_adamw_equals_the_separate_passes_bit_for_bit():
    from oracle import synth
    cfg = synth.make_config("hd64", mask_rate=0.2)
    rows = 3
    P = synth.make_params(cfg, 5, "test")
    batches = [synth.make_batch(cfg, rows, 60 + i) for i in range(2)]
    masks = [synth.make_masks(cfg, rows, 70 + i) for i in range(2)]
    a = _three_steps(cfg, P, batches, masks, "fp32", True, fused=True)
    b = _three_steps(cfg, P, batches, masks, "fp32", True, fused=False)
    for (la, ga), (lb, gb) in zip(a[0], b[0]):
        assert np.array_equal(la, lb)
    # the clip coefficient is applied inside AdamW (fused) or by a separate scale pass (unfused): same products, so the same bits
    # up to the rounding of g * coef being done once in both
    worst = max(float(np.abs(a[1][n] - b[1][n]).max() / max(np.abs(b[1][n]).max(), 1e-6)) for n in a[1])
    assert worst <= 1e-6, worst


def test_deterministic_finetune_step():
    import recommendersystem_amd as ra
    from oracle import synth
    cfg = synth.make_config("hd64", mask_rate=0.2, finetune=True, finetune_metric="rating")
    rows = 3
    P = synth.make_params(cfg, 7, "test")
    batches = [synth.make_batch(cfg, rows, 80 + i) for i in range(2)]
    masks = [synth.make_masks(cfg, rows, 90 + i) for i in range(2)]
    a = _three_steps(cfg, P, batches, masks, "bf16", True)
    b = _three_steps(cfg, P, batches, masks, "bf16", True)
    assert _bitwise(a, b)


def test_benchmark_size_steps_are_bitwise_reproducible():
    """cfg-3 at the benchmark's own batch (64 rows x 512), device-drawn masks, fused clip + AdamW: two runs of two steps end with
    the same bits in every trainable tensor (129 M parameters) and the same losses."""
    import hashlib

    import recommendersystem_amd as ra
    from recommendersystem_amd import workload

    def run():
        cfg = workload.make_config("cfg3", deterministic=True)
        model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=64)
        model.init_weights(0x1217); model.random_pretrained_embeddings(0x3E7A)
        opt = ra.create_optimizer(model, cfg)
        model.set_loss_weights(ra.make_task_weights(), 1)
        d = workload.make_batch(cfg, 64, 0xD47A, mu=4.6, sigma=1.0)
        losses = []
        for _ in range(2):
            losses.append(model(d, False))
            opt.step(lr_factor=1.0, clip_max_norm=1.0)
        h = hashlib.sha256()
        for name, shape, trainable in model.named_parameters():
            if trainable:
                h.update(model.get_parameter(name).tobytes())
        model.close()
        return losses, h.hexdigest()
    (la, ha), (lb, hb) = run(), run()
    assert la == lb and ha == hb, (la, lb)


def test_data_parallel_step_on_two_concurrent_ranks_is_bitwise_reproducible():
    """Deterministic models behind the data-parallel all-reduce (early buckets armed, in-process rank group: ranks summed in rank
    order, as a ring with a fixed topology does): the reduced gradients and the updated parameters repeat bit for bit."""
    import threading

    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import dist as rdist
    from recommendersystem_amd.optim import AdamW
    cfg = synth.make_config("hd64", mask_rate=0.2, mask_topk=16, deterministic=True)
    rows, world = 2, 2
    P = synth.make_params(cfg, 23, "test")
    batches = [synth.make_batch(cfg, rows, 24 + 10 * r) for r in range(world)]
    masks = [synth.make_masks(cfg, rows, 25 + 10 * r) for r in range(world)]
    names = synth.trainable_names(cfg)

    def once():
        group = rdist.LocalGroup(world)
        out = [None] * world; err = [None] * world

        def rank_fn(r):
            try:
                comm = rdist.LocalComm(group, r)
                model = ra.RecommenderModel(cfg, dtype="bf16", max_rows=rows)
                model.load_state_dict(P)
                model.set_loss_weights(TASK_W, 1)
                comm.begin_grad_sync(model)
                losses = model(batches[r], False, masks=masks[r])
                comm.all_reduce_grads(model)
                G = {n: model.grad(n).copy() for n in names}
                AdamW(model, lr=1e-2).step(clip_max_norm=1.0, grad_div=float(world))
                Pn = {n: model.get_parameter(n).copy() for n in names}
                model.close(); comm.close()
                out[r] = (losses, G, Pn)
            except BaseException as e:   # noqa: BLE001
                err[r] = e
        th = [threading.Thread(target=rank_fn, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(300)
        group.close()
        for e in err:
            if e is not None:
                raise e
        return out
    a, b = once(), once()
    for r in range(world):
        assert a[r][0] == b[r][0]
        for n in names:
            assert np.array_equal(a[r][1][n], b[r][1][n]), (r, n)
            assert np.array_equal(a[r][2][n], b[r][2][n]), (r, n)
            assert np.array_equal(a[r][2][n], a[0][2][n]), (r, n)      # and the ranks agree with each other


@pytest.mark.parametrize("sampled", [0, 24])
def test_row_sharded_table_is_bitwise_reproducible_too(sampled):
    """Deterministic mode on the row-sharded table: the vocabulary-parallel heads sum their loss terms in row order, their split-K
    gradient goes through ordered slabs, the row exchange adds requester by requester and the in-process group reduces in rank
    order -- two runs of two optimizer steps on two concurrent ranks end with the same bits on every rank.  sampled > 0: the
    sampled soft-max, whose target-class gradient rows (shared by the rows with the same target) are then added by the first such
    row in row order (ss_target_grad_ordered_kernel) instead of by float atomics; a third run in the default mode shows that the
    ordered form computes the same gradients up to the order of the sums."""
    import threading

    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import dist as rdist
    cfg = synth.make_config("hd64", mask_rate=0.2, mask_topk=16)
    world, rows = 2, 3
    P = synth.make_params(cfg, 3, "test")
    E, M = "item_embedding.matchedid_embedding.embedding.weight", "item_embedding.metadata_embedding.embedding.weight"
    batches = [[synth.make_batch(cfg, rows, 40 + 10 * r + i) for i in range(2)] for r in range(world)]
    masks = [[synth.make_masks(cfg, rows, 50 + 10 * r + i) for i in range(2)] for r in range(world)]
    names = synth.trainable_names(cfg)

    def run(deterministic=True):
        group = rdist.LocalGroup(world)
        out = [None] * world; err = [None] * world

        def rank(r):
            try:
                comm = rdist.LocalComm(group, r)
                c = dict(cfg, deterministic=deterministic); c["table_shard"] = (r, world)
                if sampled:
                    c["sampled_softmax"] = sampled
                m = ra.RecommenderModel(c, dtype="bf16", max_rows=rows)
                m.set_shard_comm(comm)
                lo, hi = m.table_rows()
                sd = dict(P); sd[E] = P[E][lo:hi]; sd[M] = P[M][lo:hi]
                m.load_state_dict(sd)
                opt = ra.create_optimizer(m, dict(cfg, learning_rate=1e-2))
                m.set_loss_weights(TASK_W, 1)
                res = []
                for d, mk in zip(batches[r], masks[r]):
                    losses = m(d, False, masks=mk)
                    comm.all_reduce_grads(m)
                    res.append((np.array(losses, np.float32), {n: m.grad(n).copy() for n in names}))
                    opt.step(clip_max_norm=1.0, grad_div=float(world))
                out[r] = (res, {n: m.get_parameter(n).copy() for n in names})
                m.close(); comm.close()
            except BaseException as e:   # noqa: BLE001
                err[r] = e
        th = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(300)
        group.close()
        for e in err:
            if e is not None:
                raise e
        return out
    a, b = run(), run()
    for r in range(world):
        assert _bitwise(a[r], b[r]), r
    if sampled:
        c = run(deterministic=False)
        shared = 0
        for r in range(world):
            for (la, ga), (lc, gc) in zip(a[r][0], c[r][0]):
                assert np.allclose(la, lc, rtol=2e-3), (la, lc)
                for n in names:
                    assert np.abs(ga[n] - gc[n]).max() <= 2e-2 * max(np.abs(gc[n]).max(), 1e-6), n
        for i in range(2):         # (and the case the ordered kernel exists for did occur: live rows that share a watch target)
            for med in (0, 1):
                lab = np.concatenate([np.asarray(batches[r][i][f"{med}.watch.label"]).reshape(-1) for r in range(world)])
                wgt = np.concatenate([np.asarray(batches[r][i][f"{med}.watch.weight"]).reshape(-1) for r in range(world)])
                live = lab[wgt > 0]
                shared += int(len(live) - len(np.unique(live)))
        assert shared > 0


def test_benchmark_size_attention_backward_is_bitwise_reproducible():
    """rsys_op_attention at the benchmark's shape (64 rows of 1024 tokens, 8 heads on 4 kv heads, hd 64: the paired-head
    kernels), sixteen times on the same operands: O, the log-sum-exp and dQ/dK/dV must come back identical every time.  The
    kernels have no atomics, so anything else is a fault: in round 4 sixteen queries x one column of dQ came back with the
    o2*cos product of the un-rotation missing about once per three launches, when the build still let the compiler pack that
    arithmetic into v_pk_fma_f32 with a crossed low half (csrc/Makefile, profiles/r4_attn_dq_packed_f32_glitch.log)."""
    import ctypes as C
    from recommendersystem_amd import _lib, workload
    lib = _lib.lib()
    cfg = workload.make_config("cfg3")
    B, S, H, KV = 64, cfg["max_sequence_length"], cfg["num_heads"], cfg["num_kv_heads"]
    hd, T = cfg["embed_dim"] // H, 2 * S
    d = workload.make_batch(cfg, B, 0xD47A, mu=4.6, sigma=1.0)
    rng = np.random.default_rng(0)
    uid = np.repeat(np.asarray(d["userid"], np.int32).reshape(-1), 2)
    tm = np.repeat((np.asarray(d["token_mask_ids"]).reshape(-1) * (rng.random(B * S) < 0.1)).astype(np.int32), 2)
    Nq = (H + 2 * KV) * hd
    held = []

    def dev(a):
        p = C.c_void_p()
        _lib.check(lib.rsys_dev_alloc(C.byref(p), a.nbytes))
        lib.rsys_dev_h2d(p, a.ctypes.data, a.nbytes)
        held.append(p)
        return p

    bf = lambda a: (np.ascontiguousarray(a, np.float32).view(np.uint32) >> 16).astype(np.uint16)
    qkv, dO = dev(bf(rng.standard_normal((B * T, Nq)))), dev(bf(rng.standard_normal((B * T, H * hd))))
    d_uid, d_tm = dev(uid), dev(tm)
    ang = np.outer(np.arange(T, dtype=np.float32), 1.0 / (500000.0 ** (np.arange(0, hd, 2, dtype=np.float32) / hd)))
    cos, sin = dev(np.cos(ang).astype(np.float32)), dev(np.sin(ang).astype(np.float32))
    O, dq, lse = dev(np.zeros((B * T, H * hd), np.uint16)), dev(np.zeros((B * T, Nq), np.uint16)), dev(np.zeros((B, H, T), np.float32))
    first = None
    try:
        for rep in range(16):
            _lib.check(lib.rsys_op_attention(1, B, T, H, KV, hd, qkv, d_uid, d_tm, O, lse, dO, dq, cos, sin))
            got = [np.empty((B * T, H * hd), np.uint16), np.empty((B * T, Nq), np.uint16), np.empty((B, H, T), np.float32)]
            for a, p in zip(got, (O, dq, lse)):
                lib.rsys_dev_d2h(a.ctypes.data, p, a.nbytes)
            if first is None:
                first = got
                assert np.abs(got[2]).max() > 0 and (got[1] != 0).any()
                continue
            for name, a, b in zip(("O", "dqkv", "lse"), first, got):
                bad = np.argwhere(a != b)
                assert len(bad) == 0, f"launch {rep}: {name} differs from launch 0 in {len(bad)} elements, first at {bad[0].tolist()}"
    finally:
        for p in held:
            lib.rsys_dev_free(p)


def test_bench_dump_outputs_agree_between_two_runs(tmp_path):
    """bench.py --dump-outputs, run twice with the same arguments: the replayed steps before the last are bitwise reproducible, so the
    last one (on the timed path, float atomics included) starts from the same bits and its outputs agree to float-atomic noise -- where
    the last timed step itself, after the atomics of every earlier step had compounded through AdamW, moved some weights by percents."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    for k in range(2):
        out = tmp_path / str(k)
        subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--config", "cfg2", "--steps", "4", "--warmup", "2", "--no-cpu-baseline",
                        "--no-kernel-timing", "--no-train-loop", "--no-extra-legs", "--dump-outputs", str(out)],
                       check=True, cwd=root, timeout=600, stdout=subprocess.DEVNULL)
        runs.append({f.name: np.load(f) for f in out.iterdir()})
    assert runs[0].keys() == runs[1].keys() and len(runs[0]) > 80
    np.testing.assert_allclose(runs[0]["losses.npy"], runs[1]["losses.npy"], rtol=1e-5)
    for name, a in runs[0].items():
        b = runs[1][name]
        assert np.isfinite(a).all() and np.abs(a - b).max() <= 1e-4 * np.abs(a).max(), (name, float(np.abs(a - b).max()), float(np.abs(a).max()))
