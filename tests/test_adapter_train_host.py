"""CPU: the host side of training through the adapter bank -- the new entry points in header, library and Julia binding;
the packer of joint batches; the joint epoch loop's bookkeeping against four independent `train_epoch` loops on the same fake model;
the early-stop decisions and the files the run writes, read back through `serve.get_models`."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rsys_adapter_train_enable", "rsys_adapter_forward_backward", "rsys_adapter_grad_get", "rsys_adapter_zero_grad",
       "rsys_adapter_adamw_step", "rsys_adapter_adamw_state_get", "rsys_adapter_adamw_state_set"]
S = 4


def test_new_entry_points_in_header_library_and_julia_binding():
    import __graft_entry__ as ge
    from recommendersystem_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsys.h")).read(), flags=re.S)
    jl = re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "RsysHIP.jl")).read())
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", hdr), name
        assert hasattr(L, name) and name in _lib.EXPORTED, name
        assert f"(:{name}, LIB)" in jl, name


def _sub(rows, tag):
    """a sub-batch of `rows` rows whose arrays carry `tag` (so that the packed rows can be told apart)"""
    return {"userid": np.full(rows * S, tag, np.int32), "0.watch.weight": np.full((rows, S), tag, np.float32)}


def test_pack_adapter_batch_rows_slots_tasks_and_absent_slots():
    from recommendersystem_amd.train import pack_adapter_batch
    batch, rs, rt = pack_adapter_batch([(0, 0, _sub(2, 10)), (1, 1, None), (5, 2, _sub(1, 12)), (3, 3, _sub(3, 13))], S)
    assert rs.dtype == np.int32 and rt.dtype == np.int32
    assert rs.tolist() == [0, 0, 5, 3, 3, 3] and rt.tolist() == [0, 0, 2, 3, 3, 3]
    assert batch["userid"].tolist() == [10] * 8 + [12] * 4 + [13] * 12
    assert batch["0.watch.weight"].shape == (24,) and batch["0.watch.weight"][8:12].tolist() == [12.0] * 4
    assert pack_adapter_batch([(0, 0, None), (1, 1, None)], S) == (None, None, None)
    for bad in ([(0, 0, {"userid": np.zeros(S + 1, np.int32)})], [(0, 0, _sub(1, 1)), (1, 1, {"userid": np.zeros(S, np.int32)})]):
        try:
            pack_adapter_batch(bad, S)
            raise AssertionError("accepted")
        except ValueError:
            pass


class FakeModel:
    """logs what the loops ask of it; a batch's tag names the slot it belongs to, its loss is a function of the tag and the call count"""

    def __init__(self, test_losses=None):
        self.log, self.calls, self.test_losses, self.eval_round = [], 0, test_losses, {}
        self.last_weight_sums = [0.0] * 4

    # ---- the single-adapter interface train_epoch uses (callable only: the plain loop)
    def set_loss_weights(self, w, accum):
        self.accum = accum

    def __call__(self, d, evaluate):
        tag = int(np.asarray(d["userid"]).reshape(-1)[0])
        slot, task = tag // 100, tag // 100
        self.log.append(("micro", slot, tag))
        self.last_weight_sums = [2.0 if i == task else 0.0 for i in range(4)]
        return [float(tag) if i == task else 0.0 for i in range(4)]

    # ---- the joint interface
    def forward_backward_adapters(self, batch, row_slot, row_task, evaluate=False, grad_scale=1.0):
        tags = np.asarray(batch["userid"]).reshape(-1, S)[:, 0]
        losses, ws = [0.0] * 4, [0.0] * 4
        seen = []
        for tag, s, t in zip(tags.tolist(), row_slot.tolist(), row_task.tolist()):
            if s in seen:
                continue
            seen.append(s)
            ws[t] = 2.0
            if evaluate:
                k = self.eval_round.get(s, 0)
                v = self.test_losses[s][min(k, len(self.test_losses[s]) - 1)]
                losses[t] = [v, v, v] if t % 2 == 1 else v
                self.eval_round[s] = k + 1
            else:
                losses[t] = float(tag)
                self.log.append(("micro", s, tag))
                assert grad_scale == 0.5
        self.last_weight_sums = ws
        return losses

    def adapter_state_dict(self, slot):
        return {f"transformers.layers.0.attn.q_proj_lora_A.weight": np.full((8, 4), slot, np.float32)}

    def state_dict(self, include_frozen=False):
        return {"norm.scale": np.ones(4, np.float32)}


class FakeOpt:
    def __init__(self, log, slot=None):
        self.log, self.slot = log, slot

    def zero_grad(self, set_to_none=True):
        pass

    def step(self, lr_factor=None, clip_max_norm=0.0, grad_div=1.0):
        if isinstance(lr_factor, dict):
            for s in sorted(lr_factor):
                self.log.append(("step", s, lr_factor[s], clip_max_norm[s]))
        else:
            self.log.append(("step", self.slot, lr_factor, clip_max_norm))


def _loaders(lengths):
    return {s: [_sub(1 + (s % 2), 100 * s + j) for j in range(n)] for s, n in lengths.items()}


def test_joint_epoch_equals_four_independent_epochs():
    """Per slot: the sequence of micro-steps (which batch), optimizer steps and LR factors of train_epoch_adapters over loaders of
    unequal length equals that of train_epoch on that slot's loader alone; two epochs, so that the schedulers carry over."""
    from recommendersystem_amd.train import AdapterRun, EarlyStopper, LambdaLR, WSDScheduler, make_task_weights, train_epoch, train_epoch_adapters
    lengths = {0: 5, 1: 2, 2: 7, 3: 4}
    sched = lambda: LambdaLR(WSDScheduler(2, 10, 0.2, 0.1))
    tw = {s: make_task_weights(s >> 1, ("watch", "rating")[s & 1]) for s in range(4)}
    joint = FakeModel()
    runs = [AdapterRun(s, s, tw[s][s], sched(), EarlyStopper(2, 0.001)) for s in range(4)]
    got = [train_epoch_adapters(joint, _loaders(lengths), FakeOpt(joint.log), runs, 2, S) for _ in range(2)]
    for s in range(4):
        solo = FakeModel()
        sc = sched()
        want = [train_epoch(solo, _loaders(lengths)[s], FakeOpt(solo.log, s), sc, tw[s], 2) for _ in range(2)]
        mine = [e for e in joint.log if e[1] == s]
        # the joint pass differentiates loss_i, the slot's own run task_weight * loss_i: same clip coefficient at max_norm / task_weight
        theirs = [e if e[0] == "micro" else (e[0], e[1], e[2], e[3] / tw[s][s]) for e in solo.log]
        assert mine == theirs, (s, mine, theirs)
        assert [e[2] for e in mine if e[0] == "step"][:3] == [0.0, 0.5, 1.0][: len([e for e in mine if e[0] == "step"])]
        for ep in range(2):
            assert got[ep][s][0] == want[ep][s] and got[ep][s][1] == 2.0 * lengths[s]
        assert runs[s].opt_steps == 2 * (lengths[s] // 2) and runs[s].scheduler.last_epoch == sc.last_epoch


def test_train_adapters_stops_per_slot_and_writes_files_get_models_reads(tmp_path):
    from recommendersystem_amd import serve
    from recommendersystem_amd.train import EarlyStopper, make_adapter_runs, train_adapters
    test_losses = {0: [5.0, 4.0, 3.0, 2.0, 1.0, 0.5], 1: [5.0, 5.0, 5.0, 5.0, 5.0, 5.0], 2: [5.0, 4.0, 4.0, 4.0, 4.0, 4.0], 3: [3.0, 2.0, 2.5, 1.0, 1.0, 1.0]}
    model = FakeModel(test_losses)
    cfg = {"max_sequence_length": S, "finetune": True}
    runs = make_adapter_runs([(s, s) for s in range(4)], cfg)
    loaders = {"training": _loaders({0: 2, 1: 2, 2: 2, 3: 2}), "test": _loaders({0: 1, 1: 1, 2: 1, 3: 1})}
    hist = train_adapters(model, FakeOpt(model.log), runs, loaders, cfg, str(tmp_path), 5, 2, log=lambda *_: None)
    for s in range(4):
        st, epochs, saved = EarlyStopper(2, 0.001), 0, -1            # what train() decides on the same scores (train.py:697-757)
        st(test_losses[s][0] * runs[s].task_weight)
        for e in range(5):
            st(test_losses[s][e + 1] * runs[s].task_weight)
            epochs += 1
            saved = e if st.save_model else saved
            if st.early_stop:
                break
        assert len(hist[s]) == epochs and runs[s].done, (s, hist[s])
        z = np.load(tmp_path / ("%d.%s.lora.npz" % (s >> 1, ("watch", "rating")[s & 1])))
        assert int(z["epoch"][0]) == saved and all(k.startswith("model/") and "lora_" in k for k in z.files if k.startswith("model/"))
        rows = open(tmp_path / ("%d.%s.csv" % (s >> 1, ("watch", "rating")[s & 1]))).read().strip().split("\n")
        assert rows[0].startswith("epoch,training_loss,test_loss,") and len(rows) == 2 + epochs
    assert [len(hist[s]) for s in range(4)] == [5, 2, 3, 5]
    # the files are those of `checkpoint dedup`: base.npz + four {m}.{metric}.lora.npz, as serve.get_models takes them
    load = lambda p: (lambda z: {k: z[k] for k in z.files})(np.load(p))

    class Loaded:
        def __init__(self, cfg, device=0, dtype="bf16", max_rows=4):
            self.trunk, self.slots = None, {}

        def load_state_dict(self, sd, strict=True):
            self.trunk = sd

        def load_adapter(self, slot, sd):
            self.slots[slot] = sd

    names = ["0.watch", "0.rating", "1.watch", "1.rating"]
    m = serve.get_models(load(tmp_path / "base.npz"), [load(tmp_path / (n + ".lora.npz")) for n in names], cfg, model_cls=Loaded)
    assert list(m.trunk) == ["norm.scale"] and sorted(m.slots) == [0, 1, 2, 3]
    assert all(float(next(iter(m.slots[s].values()))[0, 0]) == s for s in range(4))
    assert m.adapter_slots == {"0.retrieval": 0, "0.ranking": 1, "1.retrieval": 2, "1.ranking": 3}
