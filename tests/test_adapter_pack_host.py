"""CPU: the host side of training the finetune adapters on packed rows -- the premise (a finetune row is a live prefix
followed by zeros), `train.pack_adapter_rows` (placement = `serve.pack_plan`, descriptors in user order, segment-relative positions,
distinct ids, zeros between segments, exact unpacking, its two refusals), the joint epoch with `pack=True` against `pack=False` on a fake
model, and the new entry points in header, library and Julia binding."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 96


def test_new_entry_points_in_headers_library_and_julia_binding():
    import __graft_entry__ as ge
    from recommendersystem_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    strip = lambda p: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", p)).read(), flags=re.S)
    jl = re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "RsysHIP.jl")).read())
    L = _lib.lib()
    for name, hdr, julia in (("rsys_adapter_forward_backward_packed", "rsys.h", True), ("rsys_op_adapter_bank_segments", "rsys_debug.h", False)):
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", strip(hdr)), name
        assert hasattr(L, name) and name in _lib.EXPORTED, name
        if julia:
            assert f"(:{name}, LIB)" in jl, name
    doc = open(os.path.join(ROOT, "include", "rsys.h")).read()
    assert "THE CALLER GUARANTEES THE RESIDENT COLUMNS" in doc          # the contract the packer enforces


def _users(n_live, seed=3, medium=1):
    """finetune rows as the shard writer makes them: history, then one test item that carries the targets; zeros behind"""
    from recommendersystem_amd import workload
    rng = np.random.default_rng(seed)
    d = {k: np.zeros((len(n_live), S), workload.key_dtype(k)) for k in workload.batch_keys()}
    for r, n in enumerate(n_live):
        d["userid"][r, :n] = 1000 + r
        d["time"][r, :n] = 1e9 + np.cumsum(rng.random(n))
        d["matchedid"][r, :n] = rng.integers(1, 30, n)
        d["status"][r, :n] = rng.integers(0, 9, n)
        d["gender"][r, :n] = 2; d["source"][r, :n] = 1
        d["rating"][r, :n] = rng.integers(1, 11, n); d["progress"][r, :n] = rng.random(n)
        d["token_mask_ids"][r, n - 1] = 1
        for metric in ("watch", "rating"):
            d[f"{medium}.{metric}.label"][r, n - 1] = 1 + r
            d[f"{medium}.{metric}.weight"][r, n - 1] = 1
            d[f"{medium}.{metric}.position"][r, n - 1] = 5 + r
    return d


def test_premise_finetune_dataset_rows_are_a_live_prefix_and_zeros(tmp_path):
    from recommendersystem_amd import data
    live = [3, 40, 96, 17, 64, 33]
    data.write_shards(str(tmp_path / "training"), [[_users(live)]], 1)
    ds = data.FinetuneDataset(str(tmp_path / "training"), 0, 1, 4, False, 1)
    seen = 0
    for b in ds:
        assert len(b) == 27
        uid = np.asarray(b["userid"])
        for r in range(uid.shape[0]):
            n = int(np.flatnonzero(uid[r])[-1]) + 1
            assert (uid[r, :n] != 0).all() and n == live[seen]
            assert all(not np.asarray(v)[r, n:].any() for v in b.values())
            seen += 1
    assert seen == len(live)


def _subs(live_by_slot, seed=3):
    return [(slot, task, None if live is None else {k: v.reshape(-1) for k, v in _users(live, seed + slot, task >> 1).items()})
            for slot, task, live in live_by_slot]


def test_pack_adapter_rows_layout():
    from recommendersystem_amd.serve import pack_plan
    from recommendersystem_amd.train import pack_adapter_rows
    subs = _subs([(0, 0, [4, 33, 96]), (1, 1, None), (5, 2, [32, 31]), (3, 3, [5, 64, 5])])
    live = [4, 33, 96, 32, 31, 5, 64, 5]
    batch, segs = pack_adapter_rows(subs, S, 8, 4)
    plan = pack_plan(live, S, 8)
    assert len(plan) == 1
    want = {u: (row, c0) for u, row, c0 in plan[0][1]}
    rows = 1 + max(r for r, _ in want.values())
    assert segs.dtype == np.int32 and segs.shape == (8, 5) and len(batch) == 28 and all(v.shape == (rows * S,) for v in batch.values())
    # descriptors in sub-batch / user order, placed as serve.pack_plan places the live lengths
    assert segs[:, 3].tolist() == [0, 0, 0, 5, 5, 3, 3, 3] and segs[:, 4].tolist() == [0, 0, 0, 2, 2, 3, 3, 3] and segs[:, 2].tolist() == live
    assert [(int(r), int(c)) for r, c in segs[:, :2]] == [want[u] for u in range(8)]
    assert all(c0 % 32 == 0 and c0 + n <= S for _, c0, n, _, _ in segs)
    b = {k: v.reshape(rows, S) for k, v in batch.items()}
    covered = np.zeros((rows, S), bool)
    originals = [(d, r) for _, _, d in subs if d is not None for r in range(d["userid"].size // S)]
    for i, ((row, c0, n, slot, task), (d, r)) in enumerate(zip(segs, originals)):
        assert not covered[row, c0:c0 + n].any()
        covered[row, c0:c0 + n] = True
        assert (b["userid"][row, c0:c0 + n] == i + 1).all()                                   # 1 + the segment's index
        assert b["rope_input_pos"][row, c0:c0 + n].tolist() == list(range(n))                 # relative to the segment
        for k, v in d.items():                                                                # unpacking returns the user's arrays exactly
            if k != "userid":
                src = np.asarray(v).reshape(-1, S)[r]
                assert np.array_equal(b[k][row, c0:c0 + n], src[:n]) and b[k].dtype == src.dtype, k
    for k, v in b.items():
        assert not v[~covered].any(), k                                                       # zeros between segments, all 28 arrays
    assert pack_adapter_rows([(0, 0, None), (1, 1, None)], S, 8, 4) == (None, None)


def test_pack_adapter_rows_repeated_user_gets_distinct_ids_within_a_row():
    from recommendersystem_amd.train import pack_adapter_rows
    d = {k: np.concatenate([v[0], v[0], v[1]]) for k, v in _users([20, 9]).items()}              # the loader repeated user 0
    batch, segs = pack_adapter_rows([(2, 3, d)], S, 4, 4)
    assert segs[:, 0].tolist() == [0, 0, 0] and segs[:, 1].tolist() == [0, 32, 64]
    uid = batch["userid"].reshape(-1, S)[0]
    assert [int(uid[c]) for c in (0, 32, 64)] == [1, 2, 3]


def test_pack_adapter_rows_refusals():
    from recommendersystem_amd.train import pack_adapter_rows
    good = _users([20, 9])
    flat = lambda d: {k: v.reshape(-1) for k, v in d.items()}
    hole = {k: v.copy() for k, v in good.items()}; hole["userid"][0, 5] = 0                     # not a prefix
    tail = {k: v.copy() for k, v in good.items()}; tail["rating"][1, 50] = 3.0                  # something behind the prefix
    empty = {k: v.copy() for k, v in good.items()}
    for v in empty.values():
        v[1] = 0
    for bad in (hole, tail, empty):
        with pytest.raises(ValueError, match="live prefix"):
            pack_adapter_rows([(0, 2, flat(bad))], S, 4, 4)
    with pytest.raises(ValueError, match="whole rows"):
        pack_adapter_rows([(0, 2, {k: v.reshape(-1)[:-1] for k, v in good.items()})], S, 4, 4)
    with pytest.raises(ValueError, match="other arrays"):
        pack_adapter_rows([(0, 2, flat(good)), (1, 3, {"userid": good["userid"].reshape(-1)})], S, 4, 4)
    with pytest.raises(ValueError, match="more than 1 packed rows"):
        pack_adapter_rows([(0, 2, flat(_users([90, 90])))], S, 1, 4)
    # the selection's capacity: 3 users with one target each in ONE packed row hold 3 > mask_topk x rows = 2 x 1 positions of task 2
    three = flat(_users([20, 9, 30]))
    with pytest.raises(ValueError, match="the selection holds 2 x 1"):
        pack_adapter_rows([(0, 2, three)], S, 4, 2)
    assert pack_adapter_rows([(0, 2, three)], S, 4, 3)[1].shape == (3, 5)


class FakeModel:
    """logs the micro-steps; a user's first time stamp names its slot's batch (test_adapter_train_host.py's tags)"""
    max_rows = 4
    config = {"mask_topk": 4}

    def __init__(self):
        self.log, self.last_weight_sums = [], [0.0] * 4

    def _losses(self, tags, slots, tasks, evaluate, grad_scale):
        losses, ws, seen = [0.0] * 4, [0.0] * 4, []
        for tag, s, t in zip(tags, slots, tasks):
            if s in seen:
                continue
            seen.append(s)
            ws[t] = 2.0
            losses[t] = ([1.0, 1.0, 1.0] if t % 2 == 1 else 1.0) if evaluate else float(tag)
            if not evaluate:
                self.log.append(("micro", s, tag))
                assert grad_scale == 0.5
        self.last_weight_sums = ws
        return losses

    def forward_backward_adapters(self, batch, row_slot, row_task, evaluate=False, grad_scale=1.0):
        tags = np.asarray(batch["gender"]).reshape(-1, S)[:, 0].tolist()
        self.log.append(("rows", len(tags)))
        return self._losses(tags, row_slot.tolist(), row_task.tolist(), evaluate, grad_scale)

    def forward_backward_adapters_packed(self, batch, segments, evaluate=False, grad_scale=1.0):
        g = np.asarray(batch["gender"]).reshape(-1, S)
        self.log.append(("rows", g.shape[0]))
        return self._losses([int(g[r, c0]) for r, c0, _, _, _ in segments], segments[:, 3].tolist(), segments[:, 4].tolist(), evaluate, grad_scale)


class FakeOpt:
    def __init__(self, log):
        self.log = log

    def zero_grad(self, set_to_none=True):
        pass

    def step(self, lr_factor=None, clip_max_norm=0.0, grad_div=1.0):
        for s in sorted(lr_factor):
            self.log.append(("step", s, lr_factor[s], clip_max_norm[s]))


def _loaders(lengths):
    out = {}
    for s, n in lengths.items():
        out[s] = []
        for j in range(n):
            d = _users([7 + s, 20][: 1 + (s % 2)], seed=10 * s + j, medium=s >> 1)
            d["gender"][d["userid"] != 0] = 100 * s + j                       # the batch's tag, on every live column
            out[s].append({k: v.reshape(-1) for k, v in d.items()})
    return out


def test_joint_epoch_with_pack_gives_the_events_of_the_unpacked_epoch():
    from recommendersystem_amd.train import AdapterRun, EarlyStopper, LambdaLR, WSDScheduler, evaluate_adapters, make_task_weights, train_epoch_adapters
    lengths = {0: 5, 1: 2, 2: 7, 3: 4}
    tw = {s: make_task_weights(s >> 1, ("watch", "rating")[s & 1]) for s in range(4)}
    logs, results, evals = {}, {}, {}
    for pack in (False, True):
        model = FakeModel()
        runs = [AdapterRun(s, s, tw[s][s], LambdaLR(WSDScheduler(2, 10, 0.2, 0.1)), EarlyStopper(2, 0.001)) for s in range(4)]
        results[pack] = [train_epoch_adapters(model, _loaders(lengths), FakeOpt(model.log), runs, 2, S, log=model.log.append, pack=pack) for _ in range(2)]
        evals[pack] = evaluate_adapters(model, _loaders(lengths), runs, S, pack=pack)
        logs[pack] = model.log
    events = lambda log: [e for e in log if e[0] != "rows"]
    assert events(logs[True]) == events(logs[False]) and len(events(logs[True])) > 30
    assert results[True] == results[False] and evals[True] == evals[False]
    rows = lambda log: [e[1] for e in log if e[0] == "rows"]
    assert len(rows(logs[True])) == len(rows(logs[False])) and sum(rows(logs[True])) < sum(rows(logs[False]))     # fewer rows, the same passes
