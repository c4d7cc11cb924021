"""Shared by the trimmed-inference tests (inputs only, no model arithmetic): users with an exact number of projected history tokens
built on tests/_adapter_bank_util.make_user, and the small serving configuration (hd64 dimensions at max_sequence_length 128)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _adapter_bank_util as ab  # noqa: E402

S_TEST = 128
# live columns of a retrieval row (history + the query token) -> the row length `trim` runs it at: one tile mostly dead; one tile exactly
# full; one live column in the second tile; three tiles (an odd count); the full row (must be the ordinary upload)
LIVE_TO_ROW_LEN = {4: 32, 32: 32, 33: 64, 91: 96, 128: 128}


def config(S=S_TEST, name="hd64", **kw):
    from oracle import synth
    cfg = synth.make_config(name, mask_rate=0.2, mask_topk=4, max_sequence_length=S, **kw)
    cfg["forward"] = "inference"
    return cfg, (cfg["vocab_sizes"]["0_matchedid"], cfg["vocab_sizes"]["1_matchedid"])


def user_with_history(rng, n_hist, cands, n_items=25):
    """ab.make_user cut to the shortest event prefix whose tokenised + projected history has exactly n_hist tokens (consecutive events
    on one item collapse into one token, so a few more events than tokens are drawn)"""
    from recommendersystem_amd import serve
    u = ab.make_user(rng, n_hist + 16 + n_hist // 8, cands, n_items)
    k = n_hist
    while len(serve.project(serve.tokenize(u["items"][:k]))) < n_hist:
        k += 1
    u["items"] = u["items"][:k]
    assert len(serve.project(serve.tokenize(u["items"]))) == n_hist
    return u


def make_model(cfg, kind, dtype, max_rows=4, seed=31):
    """(model, parameters, adapters): a plain model, or the four-adapter bank of serve.get_models"""
    import recommendersystem_amd as ra
    from oracle import synth
    from recommendersystem_amd import serve
    P = synth.make_params(cfg, seed, "test")
    adapters = ab.make_adapters(cfg, 4, 70)
    if kind == "bank":
        blobs = ab.finetune_blobs(cfg, P, adapters)
        model = serve.get_models(blobs[0], blobs, cfg, dtype=dtype, max_rows=max_rows)
    else:
        model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=max_rows)
        model.load_state_dict(P)
    return model, P, adapters


def oracle_predict(cfg, P, adapters, kind, users, task, medium):
    """serve.predict restated on the fp64 oracle: the rows serve.build_batch builds, full length"""
    from oracle import model_np
    from recommendersystem_amd import serve
    V0 = cfg["vocab_sizes"]["0_matchedid"]
    ocfg, params = cfg, P
    if kind == "bank":
        ocfg = ab.finetune_config(cfg)
        params = dict(P, **adapters[ab.SLOT_MAP[f"{medium}.{task}"]])
    mul, mri = serve._request_lengths(type("M", (), {"config": cfg})(), task, None, None)
    d = serve.build_batch(users, task, medium, V0, mul, mri)
    out = model_np.OracleModel(ocfg, params, np.float64).inference({k: np.asarray(v) for k, v in d.items()}, task)
    return [np.asarray(r[f"{medium}.{task}"], np.float64) for r in serve.extract(out, users, task, medium, mul)]


def translate_token_index(index, S, row_len):
    """Restatement (tests only) of what the library does with `token_index` on a trimmed batch: row * 2S + t -> row * 2 row_len + t; a token
    at or behind 2 row_len has no place in the trimmed rows (ValueError here, RSYS_ERR_ARG there)."""
    index = np.asarray(index, np.int64).reshape(-1)
    r, t = index // (2 * int(S)), index % (2 * int(S))
    if (t >= 2 * int(row_len)).any():
        raise ValueError("a selected token lies at or behind 2 * row_len")
    return (r * 2 * int(row_len) + t).astype(np.int32)
