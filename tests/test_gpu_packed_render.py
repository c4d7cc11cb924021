"""GPU: the render pipelines with a packed retrieval stage (rsys_serving_pack_set, serve.render_users pack=True) against
pack=False on one model: states of both media, 1-3 users each, histories of 0-11 events, one of 40-80 and one empty (the states of
tests/test_gpu_render_request.py at max_sequence_length 128, max_rows 4).

Pages and totals are equal.  "queries" and "r_masked" are held to the criteria of tests/test_gpu_packed_inference.py: max |packed - unpacked|
is measured, DESIGN.md 4zb records 0.0, so equality is asserted -- which makes the packed values' error against any reference the unpacked
values' error, inside the factor 2 the accuracy criterion allows; the queries' error against the fp64 oracle is printed for both.
"forward_rows" shows fewer retrieval forwards over fewer tokens; full-history: the kept history rows, as the store forwards read them, are
the unpacked run's."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _trim_util as tu  # noqa: E402

pytestmark = pytest.mark.gpu

_COLS = ("time", "userid", "token_mask_ids", "gender", "source", "matchedid", "status", "rating", "progress", "rope_input_pos")
KEPT_ARRAYS = {False: tuple(f"batch.{c}" for c in _COLS),
               True: tuple(f"{b}.{c}" for b in ("batch", "store", "cand") for c in _COLS) + ("cand.token_index", "store.rows")}


def relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["base", "bank"])
@pytest.mark.parametrize("full_history", [False, True], ids=["split", "full"])
def test_render_users_packed(full_history, kind, dtype):
    import test_gpu_render_request as rq
    from recommendersystem_amd import serve
    cfg, V = tu.config()
    model, P, adapters = tu.make_model(cfg, kind, dtype, max_rows=4)
    try:
        S = cfg["max_sequence_length"]
        rq._tables(model, V)
        states, pags, registry = rq._request()
        states[0]["users"][0]["user"]["items"] = []                        # a user with an empty history
        model.render_keep(True)
        assert model.serving_pack is False                                 # default off
        res, kept = {}, {}
        for pack in (False, True):
            res[pack] = serve.render_users(model, states, pags, registry, full_history=full_history, pack=pack)
            kept[pack] = {k: model.render_kept(k).copy() for k in ("forwards", "queries", "forward_rows", "r_masked", "token_index", "rows") + KEPT_ARRAYS[full_history]}
            assert model.serving_pack is False and model.serving_trim is False
        for (pa, ta), (pb, tb) in zip(res[False], res[True]):
            assert np.array_equal(pa, pb) and ta == tb
        # the queries against the fp64 oracle, user by user (printed), and against the unpacked run (equal)
        users = [(u["user"], int(st["medium"])) for st in states for u in st["users"]]
        ref = np.stack([tu.oracle_predict(cfg, P, adapters, kind, [u], "retrieval", m)[0] for u, m in users])
        D = cfg["embed_dim"]
        q_off, q_on = kept[False]["queries"].reshape(-1, D), kept[True]["queries"].reshape(-1, D)
        e_on, e_off = relerr(q_on, ref), relerr(q_off, ref)
        d_q = float(np.abs(q_on - q_off).max())
        d_r = float(np.abs(kept[True]["r_masked"] - kept[False]["r_masked"]).max()) if kept[False]["r_masked"].size else 0.0
        print(f"render full_history={full_history} {kind} [{dtype}] max |packed - unpacked| queries {d_q:.3e} r_masked {d_r:.3e}  "
              f"queries' oracle error: packed {e_on:.3e} unpacked {e_off:.3e}")
        assert e_on <= 2 * e_off
        assert np.array_equal(q_on, q_off) and np.array_equal(kept[True]["r_masked"], kept[False]["r_masked"])
        # everything after Q is in user order as before: the kept batches, records and (full) the store rows cut from the kept history rows
        for k in ("token_index", "rows") + KEPT_ARRAYS[full_history]:
            assert np.array_equal(kept[False][k], kept[True][k]), k
        if full_history:
            assert kept[True]["store.userid"].size and kept[True]["store.matchedid"].any()
        # fewer retrieval forwards over fewer tokens, and the plan is serve.pack_plan's
        fr_off, fr_on = kept[False]["forward_rows"].reshape(-1, 3), kept[True]["forward_rows"].reshape(-1, 3)
        r_off, r_on = fr_off[fr_off[:, 0] == 0], fr_on[fr_on[:, 0] == 0]
        args = serve.render_pack(states, pags, S, V[0], registry, getattr(model, "adapter_slots", None), full_history)
        live = (np.asarray(args["retrieval_token"]) // 2 + 1).tolist()
        plan = serve.pack_plan(live, S, model.max_rows)
        assert [[0, 1 + max(r for _, r, _ in placed), rl] for rl, placed in plan] == r_on.tolist()
        assert len(r_off) == -(-len(live) // model.max_rows) and len(r_on) < len(r_off)
        tok = lambda fr: int((2 * fr[:, 1] * fr[:, 2]).sum())
        assert tok(r_on) < tok(r_off)
        assert kept[True]["forwards"][0] == len(r_on) and kept[True]["forwards"][1] == kept[False]["forwards"][1]
        print(f"  retrieval forwards (rows, row_len): unpacked {r_off[:, 1:].tolist()} packed {r_on[:, 1:].tolist()}; tokens {tok(r_off)} -> {tok(r_on)}")
    finally:
        model.close()


def test_a_retrieval_row_with_two_users_is_refused():
    import recommendersystem_amd as ra
    import test_gpu_render_request as rq
    from recommendersystem_amd import serve
    cfg, V = tu.config()
    model, P, adapters = tu.make_model(cfg, "base", "fp32", max_rows=4)
    try:
        rq._tables(model, V)
        states, pags, registry = rq._request()
        args = serve.render_pack(states, pags, cfg["max_sequence_length"], V[0], registry, None, False)
        row = int(np.argmax(np.asarray(args["retrieval_token"])))
        args["retrieval_rows"]["userid"][row, 0] = 2
        model.serving_pack = True
        with pytest.raises(ra.RsysError, match="one user"):
            model.render_request(**args)
        model.serving_pack = False
        model.render_request(**args)                                       # the unpacked stage takes the rows as they are
    finally:
        model.close()
