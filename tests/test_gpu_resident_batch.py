"""GPU: what one resident batch had does not leak into the next (csrc/model_batch.hip: every way of making a batch resident goes
through one installer).  Masks, RoPE positions and the row length of batch n must not show in batch n + 1, and the K/V cache's candidate
pass must hand the resident batch its own positions back.  fp32 in deterministic mode, so every comparison is bitwise; each step is
compared against a fresh model that saw only that step's upload."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS, SEED, STEP = 3, 0x51, 5


@pytest.fixture(scope="module")
def env():
    from oracle import synth
    cfg = synth.make_config("tiny", mask_rate=0.25, mask_topk=4)
    return cfg, synth.make_params(cfg, 17, "test")


def new_model(env):
    import recommendersystem_amd as ra
    cfg, P = env
    model = ra.RecommenderModel(cfg, dtype="fp32", max_rows=ROWS)
    model.load_state_dict(P)
    model.set_deterministic(True)
    model.mask_seed = SEED
    return model


def evaluate(model):
    model.forward_resident(True, step=STEP)
    return model.losses(True)


def fresh(env, run):
    """what `run` returns on a model that has seen nothing else"""
    model = new_model(env)
    try:
        return run(model)
    finally:
        model.close()


def select_resident(model, idx, task=1):
    """rsys_infer_select over the batch that is resident now (no upload)"""
    from recommendersystem_amd import _lib
    D = model.config["embed_dim"]
    out = np.empty((idx.size, D) if task == 0 else (idx.size,), np.float32)
    _lib.check(_lib.lib().rsys_infer_select(model._h, task, idx.ctypes.data, idx.size, out.ctypes.data, out.size))
    return out


def with_positions(cfg, d, seed):
    S = cfg["max_sequence_length"]
    return dict(d, rope_input_pos=np.random.default_rng(seed).integers(0, S, d["userid"].size).astype(np.int32))


def test_masks_do_not_leak(env):
    from oracle import synth
    cfg, _ = env
    A = synth.make_batch(cfg, ROWS, 101)
    masks = synth.make_masks(cfg, ROWS, 102)
    model = new_model(env)
    model.upload(A, masks)
    explicit = evaluate(model)
    model.upload(A)
    drawn = evaluate(model)
    model.prefetch(A, masks)
    model.swap_batch()
    swapped = evaluate(model)
    model.upload(synth.make_batch(cfg, ROWS - 1, 103))          # a prefetched batch without masks behind a resident one with them
    model.prefetch(A)
    model.swap_batch()
    swapped_drawn = evaluate(model)
    model.close()
    assert explicit == swapped
    assert explicit == fresh(env, lambda m: (m.upload(A, masks), evaluate(m))[1])
    assert drawn == fresh(env, lambda m: (m.upload(A), evaluate(m))[1])
    assert swapped_drawn == drawn
    assert explicit != drawn                                       # (the masks matter at all)


def test_positions_do_not_leak(env):
    from oracle import synth
    cfg, _ = env
    B = synth.make_batch(cfg, ROWS, 111)
    Bp = with_positions(cfg, B, 112)
    model = new_model(env)
    placed = model.inference_forward(Bp, "retrieval")
    plain = model.inference_forward(B, "retrieval")
    model.close()
    assert np.array_equal(plain, fresh(env, lambda m: m.inference_forward(B, "retrieval")))
    assert np.array_equal(placed, fresh(env, lambda m: m.inference_forward(Bp, "retrieval")))
    assert not np.array_equal(placed, plain)


def test_row_length_does_not_leak(env):
    from oracle import synth
    cfg, _ = env
    S = cfg["max_sequence_length"]
    A = synth.make_batch(cfg, ROWS, 121)
    short = {k: np.array(v).copy() for k, v in synth.make_batch(cfg, ROWS, 122).items()}
    for v in short.values():
        v.reshape(ROWS, S)[:, 7:] = 0                               # live prefixes of 7 events: rows of 8
    idx = np.arange(0, 2 * 8, 3, dtype=np.int32)
    model = new_model(env)
    trimmed = model.inference_select(short, "retrieval", idx, row_len=8)
    assert model.batch_row_length == 8
    model.upload(A)
    assert model.batch_row_length == S
    full = evaluate(model)
    assert model.batch_row_length == S
    model.close()
    assert full == fresh(env, lambda m: (m.upload(A), evaluate(m))[1])
    assert np.array_equal(trimmed, fresh(env, lambda m: m.inference_select(short, "retrieval", idx, row_len=8)))


def test_the_candidate_pass_restores_the_positions(env):
    from oracle import synth
    from recommendersystem_amd import _lib
    cfg, _ = env
    S = cfg["max_sequence_length"]
    H = synth.make_batch(cfg, ROWS, 131)
    X = synth.make_batch(cfg, ROWS, 132)
    Xp = with_positions(cfg, X, 133)
    idx = np.arange(1, ROWS * 2 * S, 5, dtype=np.int32)
    i32 = lambda *x: np.array(x, np.int32)
    model = new_model(env)
    model.rank_cache_reserve(ROWS)
    model.rank_cache_store(H, [5, 9, S - 1], [0, 1, 2])
    model.upload(Xp)
    before = select_resident(model, idx)
    slots, n_cand = i32(2, 0, 1), i32(1, 4, S)
    out = np.empty(int(n_cand.sum()), np.float32)
    _lib.check(_lib.lib().rsys_rank_cache_candidates(model._h, None, slots.ctypes.data, n_cand.ctypes.data, out.ctypes.data))
    after = select_resident(model, idx)
    model.upload(X)
    plain = select_resident(model, idx)                             # ... and a batch without positions behind the pass has none
    model.close()
    assert np.isfinite(out).all()
    assert np.array_equal(before, after)
    assert np.array_equal(before, fresh(env, lambda m: (m.upload(Xp), select_resident(m, idx))[1]))
    assert np.array_equal(plain, fresh(env, lambda m: (m.upload(X), select_resident(m, idx))[1]))
    assert not np.array_equal(before, plain)
