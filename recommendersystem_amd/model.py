"""Host-side mirror of the reference's model API over the C ABI.

Mirrors notebooks/Training/transformer.model.py ("model.py") as used by
notebooks/Training/transformer.py ("train.py"):

  RecommenderModel(config)                 model.py:346-377   -> rsys_model_create
  model.load_pretrained_embeddings(...)    model.py:379-389   -> rsys_model_load_metadata
  model(d, evaluate) -> 4 losses           model.py:493-529   -> rsys_batch_upload + rsys_forward_backward
  model(d, task)  (inference)              model.py:531-538   -> rsys_infer
  state_dict()/load_state_dict()           train.py:458,664   -> rsys_param_get / rsys_param_set

Difference forced by fusing forward and backward in one device pass: the
reference computes `loss = sum(tloss[i]*task_weights[i])/grad_accum` on the host
and calls loss.backward() (train.py:264-272); here the task weights and the
1/grad_accum scale are given BEFORE the call (`set_loss_weights`) and
`model(d, False)` accumulates the gradient of that weighted sum.
All arrays are numpy; device memory is owned by the library.
"""
import ctypes as C
import itertools
import os

import numpy as np

from . import _lib
from ._lib import check, lib

ALL_MEDIUMS = [0, 1]
ALL_METRICS = ["watch", "rating"]
_METRICS3 = ["watch", "rating", "status"]
DTYPES = {"fp32": 0, "float32": 0, "f32": 0, "bf16": 1, "bfloat16": 1, "fp8": 2, "float8": 2}   # fp8: bf16 + the float8 trunk linears (transformer.py:671-676)


def _c_config(config, dtype, max_rows):
    vs = config["vocab_sizes"]
    c = _lib.rsys_config()
    c.num_layers = config["num_layers"]; c.num_heads = config["num_heads"]; c.num_kv_heads = config["num_kv_heads"]
    c.embed_dim = config["embed_dim"]; c.intermediate_dim = config["intermediate_dim"]
    c.max_sequence_length = config["max_sequence_length"]
    c.vocab_0 = vs["0_matchedid"]; c.vocab_1 = vs["1_matchedid"]
    c.vocab_status = vs["status"]; c.vocab_gender = vs["gender"]; c.vocab_source = vs["source"]
    c.metadata_dim = config["metadata_emb_size"]
    c.min_ts = float(config["min_ts"]); c.max_ts = float(config["max_ts"])
    c.rating_mean = float(config["rating_mean"]); c.rating_std = float(config["rating_std"])
    c.mask_rate = float(config["mask_rate"]); c.mask_topk = int(config["mask_topk"])
    c.finetune = 1 if config.get("finetune") else 0
    c.finetune_metric = 1 if config.get("finetune_metric") == "rating" else 0
    c.dtype = DTYPES[dtype]
    c.max_rows = int(max_rows)
    c.lora_dropout = float(config.get("lora_dropout", 0.1 if config.get("finetune") else 0.0))   # nn.Dropout(0.1), model.py:238
    shard = config.get("table_shard")            # (rank, world): row-sharded item table (cfg-4); None = replicated
    c.table_shard_rank, c.table_shard_world = (int(shard[0]), int(shard[1])) if shard else (0, 0)
    c.sampled_negatives = int(config.get("sampled_softmax", 0))   # classes sampled per rank and medium (0: full soft-max)
    return c


def precompute_freqs_cis(dim, end, theta=500000.0):
    """model.py:173-179 in float32 (host computes the tables, the device only reads them)."""
    freqs = (1.0 / (np.float32(theta) ** (np.arange(0, dim, 2, dtype=np.float32)[: dim // 2] / np.float32(dim)))).astype(np.float32)
    t = np.arange(end, dtype=np.float32)
    f = np.outer(t, freqs).astype(np.float32)
    return np.cos(f).astype(np.float32), np.sin(f).astype(np.float32)


class RecommenderModel:
    def __init__(self, config, device=0, dtype="bf16", max_rows=None):
        assert config.get("forward", "train") in ("train", "inference")
        self.config = config
        self.device = device
        self.dtype = dtype
        self.max_rows = int(max_rows if max_rows is not None else config.get("local_batch_size", 1))
        self._h = C.c_void_p()
        cc = _c_config(config, dtype, self.max_rows)
        check(lib().rsys_model_create(C.byref(cc), device, C.byref(self._h)))
        hd = config["embed_dim"] // config["num_heads"]
        cos, sin = precompute_freqs_cis(hd, 2 * config["max_sequence_length"])
        check(lib().rsys_model_set_rope(self._h, cos.ctypes.data, sin.ctypes.data, cos.shape[0]))
        self._names = None
        self._task_w = None
        self._grad_scale = 1.0
        self._keep = None
        self.training = True
        self.mask_seed = 0x3A5C
        self._step = 0
        if config.get("deterministic"):
            self.set_deterministic(True)

    # ---- lifetime
    def close(self):
        if self._h:
            lib().rsys_model_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def train(self):
        self.training = True
        return self

    def eval(self):
        self.training = False
        return self

    # ---- parameters
    def init_weights(self, seed=0x1217):
        """self.apply(init_weights), model.py:5-12,360 (device-side Philox normal)."""
        check(lib().rsys_model_init_random(self._h, seed))

    def load_pretrained_embeddings(self, table):
        """model.py:379-389; `table` is the (V, M) float32 `metadata` array of media_embeddings.h5, or, as in the
        reference, the directory that holds that file."""
        if isinstance(table, (str, os.PathLike)):
            from . import h5
            with h5.File(os.path.join(table, "media_embeddings.h5")) as f:
                table = f["metadata"]
        table = np.ascontiguousarray(table, np.float32)
        check(lib().rsys_model_load_metadata(self._h, table.ctypes.data, table.shape[0], table.shape[1]))

    def random_pretrained_embeddings(self, seed=0x3E7A):
        check(lib().rsys_model_random_metadata(self._h, seed))

    def set_deterministic(self, on=True):
        """bitwise reproducible training steps (fixed summation order everywhere; a few percent slower); also `config["deterministic"]`"""
        check(lib().rsys_model_set_deterministic(self._h, 1 if on else 0))

    def set_split_table_reduce(self, on=True):
        """opt-in (replicated table, bf16): reduce the item table's gradient in two parts -- the heads' part early and out of place
        under the trunk backward, the batch's token rows as a gathered list in the tail (`Comm.begin_grad_sync` arms it per step)"""
        check(lib().rsys_model_set_split_table_reduce(self._h, 1 if on else 0))

    def set_shard_comm(self, comm):
        """row-sharded table mode: the communicator of the row exchange and the vocabulary-parallel cross entropy"""
        check(lib().rsys_model_set_shard_comm(self._h, comm._h if comm is not None else None))

    def table_rows(self):
        """[lo, hi) of the (V + 1)-row item table held by this model"""
        lo = C.c_int64(); hi = C.c_int64()
        check(lib().rsys_table_rows(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def named_parameters(self):
        """[(name, shape, trainable)] in state_dict order."""
        if self._names is None:
            n = C.c_int32()
            check(lib().rsys_param_count(self._h, C.byref(n)))
            out = []
            for i in range(n.value):
                name = C.create_string_buffer(256)
                shape = (C.c_int64 * 2)()
                nd = C.c_int32(); tr = C.c_int32()
                check(lib().rsys_param_info(self._h, i, name, 256, C.byref(shape), C.byref(nd), C.byref(tr)))
                shp = (shape[0],) if nd.value == 1 else (shape[0], shape[1])
                out.append((name.value.decode(), tuple(int(x) for x in shp), bool(tr.value)))
            self._names = out
        return self._names

    def _shape(self, name):
        base = name[len("watch_head."):] if name.startswith("watch_head.") else name
        for n, s, _ in self.named_parameters():
            if n == base:
                return base, s
        raise KeyError(name)

    def get_parameter(self, name):
        base, shape = self._shape(name)
        out = np.empty(shape, np.float32)
        check(lib().rsys_param_get(self._h, base.encode(), out.ctypes.data, out.size))
        return out

    def set_parameter(self, name, value):
        base, shape = self._shape(name)
        v = np.ascontiguousarray(value, np.float32)
        assert v.shape == tuple(shape), (name, v.shape, shape)
        check(lib().rsys_param_set(self._h, base.encode(), v.ctypes.data, v.size))

    def grad(self, name):
        base, shape = self._shape(name)
        out = np.empty(shape, np.float32)
        check(lib().rsys_grad_get(self._h, base.encode(), out.ctypes.data, out.size))
        return out

    TABLE_KEYS = ("item_embedding.matchedid_embedding.embedding.weight", "item_embedding.metadata_embedding.embedding.weight")

    def state_dict(self, include_frozen=True, gather=None):
        """The reference's state dict.  With a row-sharded item table the two table tensors are this rank's rows; pass
        `gather` = the ranks' `dist.HostGroup` to get the full tables on every rank (checkpoints: the reference's layout)."""
        sd = {}
        for n, _, tr in self.named_parameters():
            if not include_frozen and "metadata_embedding" in n:
                continue
            sd[n] = self.get_parameter(n)
            if gather is not None and n in self.TABLE_KEYS and self.config.get("table_shard"):
                sd[n] = gather_rows(gather, sd[n])
        for k in list(sd):
            if k.startswith("item_embedding."):       # watch_head shares item_embedding (model.py:354)
                sd["watch_head." + k] = sd[k]
        return sd

    def load_state_dict(self, sd, strict=True):
        """Table tensors may be given whole ((V + 1) rows, the reference's layout): a row-sharded model keeps its rows."""
        names = [n for n, _, _ in self.named_parameters()]
        assert "item_embedding.fused_embedding" not in sd          # model.py:135-137
        lo, hi = self.table_rows()
        for n in names:
            if n in sd:
                v = np.asarray(sd[n])
                if n in self.TABLE_KEYS and v.shape[0] != hi - lo:
                    v = v[lo:hi]
                self.set_parameter(n, v)
            elif strict:
                raise KeyError(f"missing key {n}")
        if strict:
            extra = [k for k in sd if k not in names and not k.startswith("watch_head.")]
            if extra:
                raise KeyError(f"unexpected keys {extra}")

    def zero_grad(self):
        check(lib().rsys_zero_grad(self._h))

    # ---- forward / backward
    def set_loss_weights(self, task_weights, grad_accum_steps=1):
        """task weights of train.py:264-267 (order ALL_MEDIUMS x ALL_METRICS) and the 1/grad_accum scale."""
        self._task_w = [float(x) for x in task_weights]
        self._grad_scale = 1.0 / float(grad_accum_steps)

    def _c_batch(self, d, masks=None):
        """the rsys_batch record of the 27 flat arrays (+ optional masks / RoPE positions) and the arrays it points into"""
        S = self.config["max_sequence_length"]
        n = int(np.asarray(d["userid"]).size)
        assert n % S == 0, "batch must hold whole rows of max_sequence_length"
        b = _lib.rsys_batch()
        b.rows = n // S
        keep = []

        def arr(x, dt):
            a = np.ascontiguousarray(np.asarray(x).reshape(-1), dt)
            assert a.size == n
            keep.append(a)
            return a.ctypes.data

        b.userid = arr(d["userid"], np.int32); b.token_mask_ids = arr(d["token_mask_ids"], np.int32)
        b.gender = arr(d["gender"], np.int32); b.source = arr(d["source"], np.int32)
        b.matchedid = arr(d["matchedid"], np.int32); b.status = arr(d["status"], np.int32)
        b.time = arr(d["time"], np.float64); b.rating = arr(d["rating"], np.float32); b.progress = arr(d["progress"], np.float32)
        zf = np.zeros(n, np.float32); zi = np.zeros(n, np.int32)
        for m in ALL_MEDIUMS:
            for j, metric in enumerate(_METRICS3):
                k = m * 3 + j
                b.label[k] = arr(d.get(f"{m}.{metric}.label", zf), np.float32)
                b.weight[k] = arr(d.get(f"{m}.{metric}.weight", zf), np.float32)
                b.position[k] = arr(d.get(f"{m}.{metric}.position", zi), np.int32)
        if masks is not None:
            b.watch_mask = arr(masks[0], np.uint8); b.rating_mask = arr(masks[1], np.uint8)
        if "rope_input_pos" in d:
            b.rope_input_pos = arr(d["rope_input_pos"], np.int32)
        return b, keep

    def upload(self, d, masks=None):
        """to_device, train.py:178-184.  d: the 27 flat arrays (any shape with rows*S elements)."""
        b, keep = self._c_batch(d, masks)
        check(lib().rsys_batch_upload(self._h, C.byref(b)))
        self._keep = keep

    def upload_trimmed(self, d, row_len):
        """rsys_batch_upload_trimmed: `d` as `upload` takes it (rows of max_sequence_length columns) for inference rows whose live events
        are a prefix; only columns [0, row_len) of every row are checked and copied, and the forwards that follow run over rows of
        2 * row_len tokens.  row_len % 4 == 0, 4 <= row_len <= S; every column from row_len on must be padding (userid 0).  Targets and
        masks are not read.  A trimmed batch is inference-only; `row_len == S` is `upload`."""
        b, keep = self._c_batch(d)
        check(lib().rsys_batch_upload_trimmed(self._h, C.byref(b), int(row_len)))
        self._keep = keep

    def _upload_rows(self, d, row_len):
        if row_len is None:
            self.upload(d)
        else:
            self.upload_trimmed(d, row_len)

    @property
    def batch_row_length(self):
        """interactions per row of the resident batch: S after an ordinary upload, row_len after `upload_trimmed`, 0 without a batch"""
        n = C.c_int32()
        check(lib().rsys_batch_row_length(self._h, C.byref(n)))
        return n.value

    @property
    def serving_trim(self):
        """rsys_serving_trim_set: every forward of `render_request` / `render_request_full` runs at the length of its longest live row
        (whole 64-token tiles) instead of max_sequence_length.  Default off."""
        on = C.c_int32()
        check(lib().rsys_serving_trim_get(self._h, C.byref(on)))
        return bool(on.value)

    @serving_trim.setter
    def serving_trim(self, on):
        check(lib().rsys_serving_trim_set(self._h, 1 if on else 0))

    @property
    def serving_pack(self):
        """rsys_serving_pack_set: the retrieval stage of `render_request` / `render_request_full` runs several users per row (segments of
        whole 64-token tiles, one adapter slot per tile), each forward at the length of its fullest row.  Default off."""
        on = C.c_int32()
        check(lib().rsys_serving_pack_get(self._h, C.byref(on)))
        return bool(on.value)

    @serving_pack.setter
    def serving_pack(self, on):
        check(lib().rsys_serving_pack_set(self._h, 1 if on else 0))

    def serving_pack_ranking(self, on=None):
        """rsys_serving_pack_ranking_set: `render_request_full` packs its K/V-cache store rows -- waves of up to the reserved cache slots,
        several histories per store row where that saves a forward or tokens (`serve.rank_cache_pack_plan`'s store stage).  Sets the
        switch when `on` is given; returns its state.  Default off."""
        if on is not None:
            check(lib().rsys_serving_pack_ranking_set(self._h, 1 if on else 0))
        state = C.c_int32()
        check(lib().rsys_serving_pack_ranking_get(self._h, C.byref(state)))
        return bool(state.value)

    def serving_compact_top(self, on=None):
        """rsys_serving_compact_top_set: inference passes run the last layer only where its outputs are read -- the tail and the final norm
        on the selected tokens, the attention for the selected queries where they are few, and a K/V-cache store pass ends at its last
        copy (`serve.compact_top_mode` restates the rules).  Sets the switch when `on` is given; returns its state.  Default off."""
        if on is not None:
            check(lib().rsys_serving_compact_top_set(self._h, int(on)))      # (2 / 3: the measurement values of rsys.h)
        state = C.c_int32()
        check(lib().rsys_serving_compact_top_get(self._h, C.byref(state)))
        return bool(state.value)

    @property
    def can_prefetch(self):
        """rsys_batch_prefetch / rsys_batch_swap: the next batch staged and copied beside the running step (replicated table)"""
        return self.config.get("table_shard") is None and not getattr(self, "_no_prefetch", False)   # (_no_prefetch: A/B switch of the tests)

    def prefetch(self, d, masks=None):
        """Check, pack and copy the NEXT batch while the step already enqueued still runs on the device (the reference's DataLoader
        workers + non_blocking to_device, train.py:162-165,178-184); `swap_batch` makes it the resident batch."""
        b, keep = self._c_batch(d, masks)
        check(lib().rsys_batch_prefetch(self._h, C.byref(b)))

    def swap_batch(self):
        check(lib().rsys_batch_swap(self._h))

    def forward_resident(self, evaluate, step=None):
        """One pass over the batch already resident on the device (asynchronous)."""
        if step is None:
            step = self._step
            self._step += 1
        if evaluate:
            tw = None
        else:
            assert self._task_w is not None, "call set_loss_weights(task_weights, grad_accum_steps) first"
            tw = (C.c_float * 4)(*self._task_w)
        check(lib().rsys_forward_backward(self._h, 1 if evaluate else 0, tw, self._grad_scale, self.mask_seed, step))

    def losses(self, evaluate=False):
        """Synchronises; returns the reference's loss list (rating entries are 3-lists when evaluate)."""
        lo = (C.c_float * 12)(); ws = (C.c_float * 4)()
        check(lib().rsys_losses_get(self._h, C.byref(lo), C.byref(ws)))
        out = []
        for ti in range(4):
            if evaluate and ti % 2 == 1:
                out.append([float(lo[3 * ti + k]) for k in range(3)])
            else:
                out.append(float(lo[3 * ti]))
        self.last_weight_sums = [float(x) for x in ws]
        return out

    LOSS_RING = 1024

    def push_losses(self):
        """park the enqueued step's losses and weight sums on the device (no host wait); read them with drain_losses()"""
        check(lib().rsys_losses_push(self._h))

    def drain_losses(self):
        """Synchronises once; [(losses, weight_sums)] of every step parked since the last drain, in order, as losses(False) /
        last_weight_sums would have given them step by step."""
        lo = np.empty((self.LOSS_RING, 12), np.float32); ws = np.empty((self.LOSS_RING, 4), np.float32); n = C.c_int32()
        check(lib().rsys_losses_drain(self._h, lo.ctypes.data, ws.ctypes.data, self.LOSS_RING, C.byref(n)))
        out = [([float(lo[s, 3 * ti]) for ti in range(4)], [float(x) for x in ws[s]]) for s in range(n.value)]
        if out:
            self.last_weight_sums = out[-1][1]
        return out

    def __call__(self, d, evaluate_or_task, masks=None):
        if isinstance(evaluate_or_task, str):
            return self.inference_forward(d, evaluate_or_task)
        evaluate = bool(evaluate_or_task)
        self.upload(d, masks)
        self.forward_resident(evaluate)
        return self.losses(evaluate)

    def inference_forward(self, d, task):
        """model.py:531-538: "retrieval" -> (rows, 2S, D), "ranking" -> (rows, 2S, 1)."""
        self.upload(d)
        S = self.config["max_sequence_length"]; D = self.config["embed_dim"]
        rows = int(np.asarray(d["userid"]).size) // S
        if task == "retrieval":
            out = np.empty((rows, 2 * S, D), np.float32)
            check(lib().rsys_infer(self._h, 0, out.ctypes.data, out.size))
            return out
        if task == "ranking":
            out = np.empty((rows, 2 * S, 1), np.float32)
            check(lib().rsys_infer(self._h, 1, out.ctypes.data, out.size))
            return out
        raise AssertionError(task)

    def inference_select(self, d, task, token_index, adapters=None, row_len=None, tile_adapters=None):
        """The inference forward reporting only the tokens a server reads (embed.py:147-161): `token_index` = flat token indices
        in [0, rows * 2S).  "retrieval" -> (n, D) trunk outputs, "ranking" -> (n,) rating-head values (computed on those rows only).
        `adapters`: one adapter-bank slot per batch row (-1 = the base model) or one slot for every row; None = the model as it is.
        `row_len`: run the rows trimmed to that many interactions (`upload_trimmed`); `token_index` keeps the geometry row * 2S + token.
        `tile_adapters` (packed rows, `serve.build_packed`): (rows, ceil(S / 32)) slots, entry j of a row for its interactions
        [32 j, 32 j + 32), -1 = the base model; instead of `adapters`."""
        if adapters is not None and tile_adapters is not None:
            raise ValueError("inference_select: adapters (one slot per row) or tile_adapters (one per 32 interactions), not both")
        self._upload_rows(d, row_len)
        idx = np.ascontiguousarray(np.asarray(token_index).reshape(-1), np.int32)
        D = self.config["embed_dim"]
        t = {"retrieval": 0, "ranking": 1}[task]
        out = np.empty((idx.size, D) if t == 0 else (idx.size,), np.float32)
        if tile_adapters is not None:
            S = self.config["max_sequence_length"]
            rows = int(np.asarray(d["userid"]).size) // S
            tiles = np.ascontiguousarray(np.asarray(tile_adapters).reshape(-1), np.int32)
            if tiles.size != rows * -(-S // 32):
                raise ValueError(f"inference_select: {tiles.size} tile slots for {rows} batch rows of {-(-S // 32)} tiles")
            check(lib().rsys_infer_select_tiles(self._h, t, tiles.ctypes.data, idx.ctypes.data, idx.size, out.ctypes.data, out.size))
            return out
        if adapters is None:
            check(lib().rsys_infer_select(self._h, t, idx.ctypes.data, idx.size, out.ctypes.data, out.size))
            return out
        rows = int(np.asarray(d["userid"]).size) // self.config["max_sequence_length"]
        slots = np.full(rows, int(adapters), np.int32) if np.ndim(adapters) == 0 else np.ascontiguousarray(np.asarray(adapters).reshape(-1), np.int32)
        if slots.size != rows:
            raise ValueError(f"inference_select: {slots.size} adapter slots for {rows} batch rows")
        check(lib().rsys_infer_select_adapters(self._h, t, slots.ctypes.data, idx.ctypes.data, idx.size, out.ctypes.data, out.size))
        return out

    # ---- ranking cache (full-length histories: the history's K / V per layer once, the candidates against it; embed.py:74-161)
    def _row_slots(self, d, adapters):
        rows = int(np.asarray(d["userid"]).size) // self.config["max_sequence_length"]
        if adapters is None:
            return rows, None
        slots = np.full(rows, int(adapters), np.int32) if np.ndim(adapters) == 0 else np.ascontiguousarray(np.asarray(adapters).reshape(-1), np.int32)
        if slots.size != rows:
            raise ValueError(f"rank cache: {slots.size} adapter slots for {rows} batch rows")
        return rows, slots

    def rank_cache_reserve(self, n_slots):
        """n_slots cache slots of [num_layers][2S][2 num_kv_heads head_dim] values in the compute dtype (0 frees them; a new size drops
        what was stored)"""
        check(lib().rsys_rank_cache_reserve(self._h, int(n_slots)))
        self.rank_cache_slots = int(n_slots)

    def rank_cache_store(self, d, n_hist, slots, adapters=None, row_len=None):
        """The trunk forward of the history-only rows `d` (row r: n_hist[r] events, token_mask_ids 0, rope_input_pos 0 .. n_hist[r] - 1);
        every layer's K / V of row r's history tokens goes to cache slot slots[r].  `adapters` and `row_len` (>= every n_hist) as in
        `inference_select`; a slot stored from a trimmed row is the slot the full row stores."""
        self._upload_rows(d, row_len)
        rows, ad = self._row_slots(d, adapters)
        nh = np.ascontiguousarray(np.asarray(n_hist).reshape(-1), np.int32); sl = np.ascontiguousarray(np.asarray(slots).reshape(-1), np.int32)
        if nh.size != rows or sl.size != rows:
            raise ValueError(f"rank_cache_store: {nh.size} history lengths and {sl.size} slots for {rows} batch rows")
        check(lib().rsys_rank_cache_store(self._h, None if ad is None else ad.ctypes.data, nh.ctypes.data, sl.ctypes.data))

    def rank_cache_candidates(self, d, slots, n_cand, adapters=None, row_len=None):
        """The trunk forward of the candidate rows `d` (row r: n_cand[r] candidates at events 0 .. n_cand[r] - 1) against the histories
        cached in slots[r]; returns the rating head at the candidates' action tokens, (sum n_cand,) float32 in row order.  `row_len`
        (>= every n_cand): the rows run trimmed, against slots stored from rows of any length."""
        self._upload_rows(d, row_len)
        rows, ad = self._row_slots(d, adapters)
        sl = np.ascontiguousarray(np.asarray(slots).reshape(-1), np.int32); nc = np.ascontiguousarray(np.asarray(n_cand).reshape(-1), np.int32)
        if nc.size != rows or sl.size != rows:
            raise ValueError(f"rank_cache_candidates: {sl.size} slots and {nc.size} candidate counts for {rows} batch rows")
        out = np.empty(int(np.clip(nc, 0, None).sum()), np.float32)
        check(lib().rsys_rank_cache_candidates(self._h, None if ad is None else ad.ctypes.data, sl.ctypes.data, nc.ctypes.data, out.ctypes.data))
        return out

    def _segments(self, what, segments, adapters):
        seg = np.ascontiguousarray(np.asarray(segments, np.int32).reshape(-1, 4))
        if adapters is None:
            return seg, None
        ad = np.full(len(seg), int(adapters), np.int32) if np.ndim(adapters) == 0 else np.ascontiguousarray(np.asarray(adapters).reshape(-1), np.int32)
        if ad.size != len(seg):
            raise ValueError(f"{what}: {ad.size} adapter slots for {len(seg)} segments")
        return seg, ad

    def rank_cache_store_packed(self, d, segments, adapters=None, row_len=None):
        """`rank_cache_store` on packed rows: `segments` = [(row, first_column, n_hist, slot)], each one user's history alone in a run of
        whole 64-token tiles of row `row` of `d` (first_column a multiple of 32, userid distinct among the segments, token_mask_ids 0);
        the call runs event i of a segment at position i.  `adapters`: one bank slot per segment (-1 = the base model), one for all, or
        None.  Slot `slot` then holds what `rank_cache_store` stores from that history in a row of its own."""
        self._upload_rows(d, row_len)
        seg, ad = self._segments("rank_cache_store_packed", segments, adapters)
        check(lib().rsys_rank_cache_store_packed(self._h, None if ad is None else ad.ctypes.data, len(seg), seg.ctypes.data))

    def rank_cache_candidates_packed(self, d, segments, adapters=None, row_len=None):
        """`rank_cache_candidates` on packed rows: `segments` = [(row, first_column, n_cand, slot)], n_cand candidates at columns
        first_column + j of row `row` against the history cached in `slot`; several segments may read one slot.  Returns the rating head
        at the candidates' action tokens, (sum n_cand,) float32, segment after segment."""
        self._upload_rows(d, row_len)
        seg, ad = self._segments("rank_cache_candidates_packed", segments, adapters)
        out = np.empty(int(np.clip(seg[:, 2], 0, None).sum()), np.float32)
        check(lib().rsys_rank_cache_candidates_packed(self._h, None if ad is None else ad.ctypes.data, len(seg), seg.ctypes.data, out.ctypes.data))
        return out

    def rank_cache_get(self, layer, slot, n_hist):
        """test hook (rsys_debug.h): the K | V rows slot `slot` holds for `layer`, (2 n_hist, 2 num_kv_heads head_dim), float32 for an
        fp32 model, raw bf16 bit patterns (uint16) for a bf16 model; n_hist must be what was stored"""
        c = self.config
        kvw = 2 * c["num_kv_heads"] * (c["embed_dim"] // c["num_heads"])
        out = np.empty((2 * int(n_hist), kvw), np.float32 if self.dtype == "fp32" else np.uint16)
        check(lib().rsys_rank_cache_get(self._h, int(layer), int(slot), out.ctypes.data, out.nbytes))
        return out

    # ---- adapter bank (base model: several LoRA adapter sets beside one frozen trunk, Finetune/embed.py:180-255)
    ADAPTER_SLOTS = 8

    def adapter_names(self):
        """[(name, shape)] of the 4 * num_layers LoRA tensors of one adapter, in the reference's state-dict order (model.py:235-254)"""
        c = self.config
        D = c["embed_dim"]; hd = D // c["num_heads"]
        out = []
        for l in range(c["num_layers"]):
            p = f"transformers.layers.{l}.attn."
            out += [(p + "q_proj_lora_A.weight", (8, D)), (p + "q_proj_lora_B.weight", (c["num_heads"] * hd, 8)),
                    (p + "v_proj_lora_A.weight", (8, D)), (p + "v_proj_lora_B.weight", (c["num_kv_heads"] * hd, 8))]
        return out

    def load_adapter(self, slot, state_dict):
        """Loads the `lora_` tensors of `state_dict` (a finetuned model's full state dict or its LoRA-only part, as
        `load_state_dict(..., strict=False)` takes them in embed.py:196) into bank slot `slot`; every LoRA tensor must be there.
        Nothing of the model itself changes: the item table, serving tables and a later training step are unaffected."""
        names = self.adapter_names()
        missing = [n for n, _ in names if n not in state_dict]
        if missing:
            raise KeyError(f"load_adapter: missing LoRA keys {missing[:4]}{' ...' if len(missing) > 4 else ''}")
        vals = []
        for n, shape in names:
            v = np.ascontiguousarray(state_dict[n], np.float32)
            if v.shape != shape:
                raise ValueError(f"load_adapter: {n} has shape {v.shape}, expected {shape}")
            vals.append(v)
        for (n, _), v in zip(names, vals):
            check(lib().rsys_adapter_set(self._h, int(slot), n.encode(), v.ctypes.data, v.size))

    def adapter_state_dict(self, slot):
        """the LoRA tensors held in `slot`, as float32 arrays under their state-dict names (bit for bit what was loaded)"""
        sd = {}
        for n, shape in self.adapter_names():
            out = np.empty(shape, np.float32)
            check(lib().rsys_adapter_get(self._h, int(slot), n.encode(), out.ctypes.data, out.size))
            sd[n] = out
        return sd

    # ---- training through the bank: the four finetune adapters in one pass on the frozen trunk (Finetune/run.jl:9-13)
    def enable_adapter_training(self, dropout=0.1):
        """gradients, AdamW moments and per-layer activations for the bank's slots; `dropout` on the LoRA input of training passes
        (model.py:238).  May be called again to change the dropout."""
        check(lib().rsys_adapter_train_enable(self._h, float(dropout)))
        self._grad_scale_adapters = 1.0

    def forward_backward_adapters(self, d, row_slot, row_task, evaluate=False, grad_scale=1.0, step=None):
        """One joint pass: batch row r runs with bank slot row_slot[r] on task row_task[r] = medium * 2 + metric (-1 / -1: the base
        model, no loss).  d None: the batch already resident.  Training passes accumulate each slot's LoRA gradients (`adapter_grad`).
        Returns the loss list of `__call__`; `last_weight_sums` holds the tasks' weight sums."""
        if d is not None:
            self.upload(d)
        rs = np.ascontiguousarray(np.asarray(row_slot).reshape(-1), np.int32)
        rt = np.ascontiguousarray(np.asarray(row_task).reshape(-1), np.int32)
        n = C.c_int32()
        check(lib().rsys_batch_rows(self._h, C.byref(n)))       # the resident batch's own count, whichever call made it resident
        rows = n.value
        if rs.size != rows or rt.size != rows:
            raise ValueError(f"forward_backward_adapters: {rs.size} slots / {rt.size} tasks for {rows} batch rows")
        if step is None:
            step = self._step
            self._step += 1
        check(lib().rsys_adapter_forward_backward(self._h, 1 if evaluate else 0, rs.ctypes.data, rt.ctypes.data, float(grad_scale),
                                                  self.mask_seed, int(step)))
        return self.losses(bool(evaluate))

    def forward_backward_adapters_packed(self, d, segments, evaluate=False, grad_scale=1.0, step=None):
        """`forward_backward_adapters` on packed rows (`train.pack_adapter_rows`): `segments` (n, 5) int32 = (row,
        first_column, columns, slot, task), one per user, each the live prefix of that user's finetune row starting on a multiple of 32
        columns.  d None: the batch already resident.  A slot's gradient sums its segments in the order given."""
        if d is not None:
            self.upload(d)
        sg = np.ascontiguousarray(np.asarray(segments), np.int32)
        if sg.ndim != 2 or sg.shape[1] != 5:
            raise ValueError(f"forward_backward_adapters_packed: segments has shape {sg.shape}, expected (n, 5)")
        if step is None:
            step = self._step
            self._step += 1
        check(lib().rsys_adapter_forward_backward_packed(self._h, 1 if evaluate else 0, sg.ctypes.data, sg.shape[0], float(grad_scale),
                                                         self.mask_seed, int(step)))
        return self.losses(bool(evaluate))

    def adapter_grad(self, slot, name=None):
        """the fp32 gradient of one LoRA tensor of `slot`, or {name: gradient} of all of them"""
        def one(n, shape):
            out = np.empty(shape, np.float32)
            check(lib().rsys_adapter_grad_get(self._h, int(slot), n.encode(), out.ctypes.data, out.size))
            return out
        shapes = dict(self.adapter_names())
        if name is not None:
            return one(name, shapes[name])
        return {n: one(n, shape) for n, shape in shapes.items()}

    def zero_adapter_grads(self):
        check(lib().rsys_adapter_zero_grad(self._h))

    def clear_adapter(self, slot):
        check(lib().rsys_adapter_clear(self._h, int(slot)))

    def adapters_loaded(self):
        """the complete slots, ascending"""
        mask = C.c_int32()
        check(lib().rsys_adapter_slots(self._h, C.byref(mask)))
        return [s for s in range(self.ADAPTER_SLOTS) if (mask.value >> s) & 1]

    def item_embeddings(self):
        """`model.item_embedding(torch.arange(0, n_0 + n_1))` (register.py:27-29): the (V, D) table E + Wp.Meta + bp."""
        V = self.config["vocab_sizes"]["0_matchedid"] + self.config["vocab_sizes"]["1_matchedid"]
        out = np.empty((V, self.config["embed_dim"]), np.float32)
        check(lib().rsys_item_table(self._h, out.ctypes.data, out.size))
        return out

    def retrieve_topk(self, queries, medium, k, group=None, prior=None, exclude=None):
        """Retrieval candidates on the device (rsys_retrieve_topk: Finetune/embed.jl:86-90 + Inference/render.jl:240-333's scoring,
        masking and sort): `queries` (n, D) retrieval embeddings; `group` (n,) group ids in [0, n_groups) or None (one group per
        query); `prior` (n_groups, V_m) added to the scores or None; `exclude` a list of n_groups arrays of medium-local ids or None.
        Per group the best k medium-local ids by the summed log soft-max (+ prior), exclusions and -inf / NaN scores left out, ties
        by ascending id.  Returns (ids (n_groups, k) int32, scores (n_groups, k) float32, counts (n_groups,) int32); slots past
        counts[g] hold -1 / -inf."""
        q = np.ascontiguousarray(queries, np.float32)
        if q.ndim == 1:
            q = q[None, :]
        n = q.shape[0]
        gp = None if group is None else np.ascontiguousarray(group, np.int32).reshape(-1)
        if gp is not None and gp.size != n:
            raise ValueError(f"group has {gp.size} entries for {n} queries")
        ng = n if gp is None else (int(gp.max()) + 1 if gp.size else 0)
        Vm = self.config["vocab_sizes"][f"{int(medium)}_matchedid"] if medium in (0, 1) else 0
        pr = None
        if prior is not None:
            pr = np.ascontiguousarray(prior, np.float32)
            if pr.shape != (ng, Vm):
                raise ValueError(f"prior has shape {pr.shape}, expected {(ng, Vm)}")
        off = ids_x = None
        if exclude is not None:
            off, ids_x = exclusion_csr(exclude, ng)
        ids = np.empty((ng, int(k)), np.int32)
        scores = np.empty((ng, int(k)), np.float32)
        counts = np.empty(ng, np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data
        check(lib().rsys_retrieve_topk(self._h, int(medium), q.ctypes.data, n, ptr(gp), ng, ptr(pr), ptr(off), ptr(ids_x), int(k),
                                       ids.ctypes.data, scores.ctypes.data, counts.ctypes.data))
        return ids, scores, counts

    TARGET_RANK_MAXQ = 4096           # queries per rsys_retrieve_target_rank call

    def retrieve_target_rank(self, queries, medium, targets, exclude=None):
        """Finetune evaluation on the device (rsys_retrieve_target_rank, Finetune/regress.jl:193-266): per query of `queries` (n, D) the
        1-based rank of its target (`targets` (n,) medium-local ids) among the admissible items by the log soft-max score of
        `retrieve_topk` (descending, ties by ascending id; 0 when the target itself is excluded, -inf or NaN) and the target's
        log-probability, read before the exclusions.  `exclude`: one array of medium-local ids per query, or None.  Calls of more than
        4096 queries are split.  Returns (rank (n,) int32, logp (n,) float32)."""
        q = np.ascontiguousarray(queries, np.float32)
        if q.ndim == 1:
            q = q[None, :]
        n = q.shape[0]
        t = np.ascontiguousarray(targets, np.int32).reshape(-1)
        if t.size != n:
            raise ValueError(f"targets has {t.size} entries for {n} queries")
        if exclude is not None and len(exclude) != n:
            raise ValueError(f"exclude has {len(exclude)} lists for {n} queries")
        rank = np.empty(n, np.int32)
        logp = np.empty(n, np.float32)
        ptr = lambda a: None if a is None else a.ctypes.data
        for a in range(0, max(n, 1), self.TARGET_RANK_MAXQ):
            b = min(n, a + self.TARGET_RANK_MAXQ)
            off = ids_x = None
            if exclude is not None:
                off, ids_x = exclusion_csr(exclude[a:b], b - a)
            qa, ta = np.ascontiguousarray(q[a:b]), np.ascontiguousarray(t[a:b])
            ra_, la = np.empty(b - a, np.int32), np.empty(b - a, np.float32)
            check(lib().rsys_retrieve_target_rank(self._h, int(medium), qa.ctypes.data, b - a, ta.ctypes.data, ptr(off), ptr(ids_x),
                                                  ra_.ctypes.data, la.ctypes.data))
            rank[a:b], logp[a:b] = ra_, la
        return rank, logp

    # ---- whole retrieval requests (rsys_retrieve_request): serving tables loaded once, then one call per batch of requests
    def _vocab(self, medium):
        if medium not in (0, 1):
            raise ValueError("medium must be 0 or 1")
        return self.config["vocab_sizes"][f"{int(medium)}_matchedid"]

    def set_retrieval_relations(self, medium, dependencies=None, recaps=None, adaptations=None):
        """Loads the relation matrices of `medium` ("{m}.dependencies", "{m}.recaps": V_m x V_m; "{m}.adaptations": V_m x V_{1-m}) onto
        the device for `retrieve_request`.  Each is a 0-based CSC `(indptr, indices, data, shape)` tuple or any object with those
        attributes (a scipy CSC matrix); None clears that table.  Stored values must be finite and >= 0; stored zeros are dropped."""
        for kind, a in enumerate((dependencies, recaps, adaptations)):
            if a is None:
                check(lib().rsys_retrieve_relations_set(self._h, int(medium), kind, 0, 0, None, None, None))
                continue
            indptr, indices, data, shape = csc_parts(a)
            check(lib().rsys_retrieve_relations_set(self._h, int(medium), kind, int(shape[0]), int(shape[1]), indptr.ctypes.data,
                                                    indices.ctypes.data, data.ctypes.data))

    def set_item_similarity(self, medium, embeddings=None, crossproject=None):
        """Loads the item-similarity table of `medium` for `retrieve_request`'s prior: `embeddings` (V_m, dim), row i = item i's vector
        (Julia's "embeddings.{m}" is its transpose, dim x V_m), `crossproject` (dim, dim) the matrix that maps a vector of `medium` into
        the other medium (x -> crossproject @ x, Julia's "crossproject.{m}") or None.  embeddings None clears both."""
        if embeddings is None:
            check(lib().rsys_retrieve_similarity_set(self._h, int(medium), 0, None, None))
            return
        e = np.ascontiguousarray(embeddings, np.float32)
        if e.ndim != 2 or e.shape[0] != self._vocab(medium):
            raise ValueError(f"embeddings have shape {e.shape}, expected ({self._vocab(medium)}, dim)")
        c = None
        if crossproject is not None:
            c = np.asfortranarray(crossproject, np.float32)                  # column-major, as Julia holds it
            if c.shape != (e.shape[1], e.shape[1]):
                raise ValueError(f"crossproject has shape {c.shape}, expected {(e.shape[1], e.shape[1])}")
        check(lib().rsys_retrieve_similarity_set(self._h, int(medium), e.shape[1], e.ctypes.data, None if c is None else c.ctypes.data))

    def set_released(self, medium, ids_or_mask=None):
        """The released items of `medium` (render.jl keeps only `keys(get_media_info(m))`): a boolean mask over [0, V_m) or an array
        of medium-local ids; None: every item is released."""
        if ids_or_mask is None:
            check(lib().rsys_retrieve_released_set(self._h, int(medium), None))
            return
        Vm = self._vocab(medium)
        a = np.asarray(ids_or_mask)
        if a.dtype == np.bool_:
            if a.shape != (Vm,):
                raise ValueError(f"released mask has shape {a.shape}, expected ({Vm},)")
            mask = a.astype(np.uint8)
        else:
            ids = a.astype(np.int64).reshape(-1)
            if ids.size and (ids.min() < 0 or ids.max() >= Vm):
                raise ValueError(f"released ids must be in [0, {Vm})")
            mask = np.zeros(Vm, np.uint8)
            mask[ids] = 1
        check(lib().rsys_retrieve_released_set(self._h, int(medium), np.ascontiguousarray(mask).ctypes.data))

    def set_query_weights(self, user_weights=None, selected_weights=None):
        """rsys_query_weights_set: a finite float32 weight per user and per selected item (flat, in the order of the request's users and
        of its selected items) for the NEXT request call on this model, which consumes them.  None = unweighted for that
        kind; both None clears what is held.  The request methods call this themselves from `user_weights=` / `selected_weights=`, and
        not at all when both are None -- the unweighted path."""
        uw = None if user_weights is None else query_weights_array(user_weights)
        sw = None if selected_weights is None else query_weights_array(selected_weights)
        uw = None if uw is None or uw.size == 0 else uw
        sw = None if sw is None or sw.size == 0 else sw
        ptr = lambda a: None if a is None else a.ctypes.data
        check(lib().rsys_query_weights_set(self._h, ptr(uw), 0 if uw is None else uw.size, ptr(sw), 0 if sw is None else sw.size))

    def query_weights_pending(self):
        """rsys_query_weights_pending: (n_users, n_sel) of the weights held for the next request, 0 = none of that kind"""
        out = np.zeros(2, np.int64)
        check(lib().rsys_query_weights_pending(self._h, out.ctypes.data))
        return int(out[0]), int(out[1])

    def query_texts_set(self, search_model, medium, x, group, weights=None):
        """rsys_query_texts_set: text queries for the NEXT request call on this model.  `x` (n, Q) float32 embeddings of
        `search_model` (a SearchModel whose features are medium `medium`'s item table, on this model's device), `group` the group of the
        consuming call per text, `weights` one finite float32 per text (None: 1.0 each).  The call scores the texts against the medium's
        items on the device and the model holds the rows until the next request call, which consumes both media's sets.  n == 0 clears
        the medium's set."""
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim == 1:
            x = x[None, :]
        n = x.shape[0]
        g = np.ascontiguousarray(group, np.int32).reshape(-1)
        if g.size != n:
            raise ValueError(f"group has {g.size} entries for {n} texts")
        w = None if weights is None else query_weights_array(weights)
        if w is not None and w.size != n:
            raise ValueError(f"weights has {w.size} entries for {n} texts")
        check(lib().rsys_query_texts_set(self._h, None if search_model is None else search_model.h, int(medium), x.ctypes.data, n,
                                         g.ctypes.data, None if w is None else w.ctypes.data))

    def query_texts_pending(self):
        """rsys_query_texts_pending: the texts held per medium for the next request, 0 = none"""
        out = np.zeros(2, np.int64)
        check(lib().rsys_query_texts_pending(self._h, out.ctypes.data))
        return int(out[0]), int(out[1])

    def _weights_before(self, user_weights, selected_weights):
        if user_weights is not None or selected_weights is not None:
            self.set_query_weights(user_weights, selected_weights)

    def retrieve_request(self, queries, medium, k, group=None, histories=None, selected=None, user_weights=None, selected_weights=None):
        """A whole render.jl `retrieval(state)` per group on the device (rsys_retrieve_request): the scores of `retrieve_topk` plus the
        item-similarity prior of the group's selected items, with the relation masks, item 0, the selected items and unreleased items
        masked, from the tables loaded by set_retrieval_relations / set_item_similarity / set_released.  `histories`: one list per query
        of (medium, id, status) list items in list order (None: no lists); `selected`: one list per group of (medium, id) items in
        the request's order (None: none).  `user_weights` (one per query) / `selected_weights` (flat, one per selected item): the query
        weights of `set_query_weights`, set immediately before the request (None: unweighted, the setter is not called).
        Returns (ids (n_groups, k) int32, scores (n_groups, k) float32, counts (n_groups,) int32)."""
        q = np.ascontiguousarray(queries, np.float32)
        if q.ndim == 1:
            q = q[None, :]
        n = q.shape[0]
        gp = None if group is None else np.ascontiguousarray(group, np.int32).reshape(-1)
        if gp is not None and gp.size != n:
            raise ValueError(f"group has {gp.size} entries for {n} queries")
        ng = n if gp is None else (int(gp.max()) + 1 if gp.size else 0)
        h = None
        if histories is not None:
            if len(histories) != n:
                raise ValueError(f"histories has {len(histories)} lists for {n} queries")
            h = triples_csr(histories, 3)
        sl = None
        if selected is not None:
            if len(selected) != ng:
                raise ValueError(f"selected has {len(selected)} lists for {ng} groups")
            sl = triples_csr(selected, 2)
        ids = np.empty((ng, int(k)), np.int32)
        scores = np.empty((ng, int(k)), np.float32)
        counts = np.empty(ng, np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data
        hp = (None,) * 4 if h is None else tuple(ptr(a) for a in h)
        sp = (None,) * 3 if sl is None else tuple(ptr(a) for a in sl)
        self._weights_before(user_weights, selected_weights)
        check(lib().rsys_retrieve_request(self._h, int(medium), q.ctypes.data, n, ptr(gp), ng, *hp, *sp, int(k), ids.ctypes.data,
                                          scores.ctypes.data, counts.ctypes.data))
        return ids, scores, counts

    WINDOW_ROWS = 1024                # ranks per window row of rsys_retrieve_window

    def retrieve_window(self, queries, medium, starts, lengths, group=None, n_groups=None, histories=None, selected=None,
                        user_weights=None, selected_weights=None):
        """`retrieve_request` for any rank range (rsys_retrieve_window): per group the items of ranks [starts[g], starts[g] + lengths[g])
        of its ordering (0-based, 1 <= length <= 1024) and its exact number of admissible items.  A group may have no queries (a state
        without users: scored by the prior of its selected items alone, no relation masks); `queries` may be None or empty, `group` then
        too.  `n_groups` defaults to len(starts).  `user_weights` / `selected_weights` as `retrieve_request`.  Returns (ids (n_groups, 1024) int32, scores (n_groups, 1024) float32, counts, totals
        (n_groups,) int32 each); slots past counts[g] = clamp(totals[g] - starts[g], 0, lengths[g]) hold -1 / -inf."""
        q = None if queries is None else np.ascontiguousarray(queries, np.float32)
        if q is not None and q.ndim == 1:
            q = q[None, :]
        n = 0 if q is None else q.shape[0]
        if n == 0:
            q = None
        ws = np.ascontiguousarray(starts, np.int64).reshape(-1)
        wl = np.ascontiguousarray(lengths, np.int32).reshape(-1)
        ng = ws.size if n_groups is None else int(n_groups)
        if ws.size != ng or wl.size != ng:
            raise ValueError(f"retrieve_window: starts and lengths need {ng} entries, one per group")
        gp = None if group is None or n == 0 else np.ascontiguousarray(group, np.int32).reshape(-1)
        if gp is not None and gp.size != n:
            raise ValueError(f"group has {gp.size} entries for {n} queries")
        if gp is None and n not in (0, ng):
            raise ValueError(f"retrieve_window: without group, {n} queries need {n} groups, not {ng}")
        h = None
        if histories is not None and n:
            if len(histories) != n:
                raise ValueError(f"histories has {len(histories)} lists for {n} queries")
            h = triples_csr(histories, 3)
        sl = None
        if selected is not None:
            if len(selected) != ng:
                raise ValueError(f"selected has {len(selected)} lists for {ng} groups")
            sl = triples_csr(selected, 2)
        ids = np.empty((ng, self.WINDOW_ROWS), np.int32)
        scores = np.empty((ng, self.WINDOW_ROWS), np.float32)
        counts = np.empty(max(ng, 1), np.int32)
        totals = np.empty(max(ng, 1), np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data
        hp = (None,) * 4 if h is None else tuple(ptr(a) for a in h)
        sp = (None,) * 3 if sl is None else tuple(ptr(a) for a in sl)
        self._weights_before(user_weights, selected_weights)
        check(lib().rsys_retrieve_window(self._h, int(medium), ptr(q), n, ptr(gp), ng, *hp, *sp, ptr(ws), ptr(wl), ids.ctypes.data,
                                         scores.ctypes.data, counts.ctypes.data, totals.ctypes.data))
        return ids, scores, counts[:ng], totals[:ng]

    def render_items(self, group_medium, offsets, limits, penalties, selected=None, selected_weights=None):
        """rsys_render_items: a page per state WITHOUT users (compute.jl `/add_item`) in one device call -- per group (medium, offset,
        limit, penalties (4)) and its selected items [(medium, id), ...]: the windowed retrieval on the item-similarity prior, then the
        reranking on zero ranking scores.  `selected_weights` as `retrieve_request`.  Returns (one int32 page array per group, exact
        totals (n_groups,) int32)."""
        gm = np.ascontiguousarray(group_medium, np.int32).reshape(-1)
        ng = gm.size
        off = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        lim = np.ascontiguousarray(limits, np.int32).reshape(-1)
        pen = np.ascontiguousarray(penalties, np.float32).reshape(-1)
        if off.size != ng or lim.size != ng or pen.size != 4 * ng:
            raise ValueError(f"render_items: offsets, limits and penalties need {ng} entries and {ng} x 4 values")
        sel = None
        if selected is not None:
            if len(selected) != ng:
                raise ValueError(f"selected has {len(selected)} lists for {ng} groups")
            sel = triples_csr(selected, 2)
        cap = int(np.clip(lim, 0, None).sum())
        ids = np.empty(max(cap, 1), np.int32)
        ioff = np.empty(ng + 1, np.int64)
        total = np.empty(max(ng, 1), np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data
        sp = (None,) * 3 if sel is None else tuple(ptr(a) for a in sel)
        self._weights_before(None, selected_weights)
        check(lib().rsys_render_items(self._h, ng, ptr(gm), ptr(off), ptr(lim), ptr(pen), *sp, ptr(ids), cap, ptr(ioff), ptr(total)))
        return [ids[ioff[g]:ioff[g + 1]].copy() for g in range(ng)], total[:ng].copy()

    # ---- ranking and reranking of retrieved candidates (rsys_rank_request: Inference/render.jl:335-435)
    def set_related(self, medium, related=None):
        """Loads "{m}.related" (V_m x V_m, a 0-based CSC `(indptr, indices, data, shape)` tuple or an object with those attributes) onto
        the device for `rank_request`'s same-series and related penalties; None clears it.  Values as `set_retrieval_relations`."""
        if related is None:
            check(lib().rsys_rank_related_set(self._h, int(medium), 0, None, None, None))
            return
        indptr, indices, data, shape = csc_parts(related)
        if shape[0] != shape[1]:
            raise ValueError(f"related has shape {shape}, expected a square V_m x V_m matrix")
        check(lib().rsys_rank_related_set(self._h, int(medium), int(shape[1]), indptr.ctypes.data, indices.ctypes.data, data.ctypes.data))

    def rank_request(self, queries, medium, candidates, group=None, r_masked=None, partialk=None, penalties=None, histories=None,
                     retrieval_coef=None, rating_coefs=None, rating_mean=0.0, scores=None, rerank=True, user_weights=None):
        """render.jl `ranking` + `reranking!` per group on the device (rsys_rank_request).  `candidates`: one array of distinct medium-local
        ids per group (1..1024 each); `queries` (n_users, D) the users' "{m}.retrieval" embeddings; `group` (n_users,) group ids or None
        (one group per user); `r_masked`: one array per user of its group's candidates' rating-head values; `partialk`: rounds per group;
        `penalties`: per group (decay, mmr_penalty, same_series_penalty, related_penalty); `histories`: per user (medium, id, status) list
        items or None; `retrieval_coef`, `rating_coefs` (c0, c1), `rating_mean`: the registry's (None: p = softmax, r = r_masked);
        `scores`: one given ranking-score array per group instead of computing them (queries and r_masked are then not needed);
        rerank=False: ranking only; `user_weights` (one per user) as `retrieve_request`.  Returns (ids per group in pick order, min(partialk, n) each, or None; ranking scores per group)."""
        ng = len(candidates)
        cand = [np.asarray(c, np.int64).reshape(-1) for c in candidates]
        off = np.zeros(ng + 1, np.int64)
        off[1:] = np.cumsum([c.size for c in cand])
        ids_in = np.ascontiguousarray(np.concatenate(cand) if ng else np.zeros(0), np.int32)
        N = int(off[-1])
        q = None
        if queries is not None:
            q = np.ascontiguousarray(queries, np.float32)
            if q.ndim == 1:
                q = q[None, :]
        nu = q.shape[0] if q is not None else (len(np.asarray(group).reshape(-1)) if group is not None else ng)
        gp = None if group is None else np.ascontiguousarray(group, np.int32).reshape(-1)
        if gp is not None and gp.size != nu:
            raise ValueError(f"group has {gp.size} entries for {nu} users")
        rm = None
        if r_masked is not None:
            if len(r_masked) != nu:
                raise ValueError(f"r_masked has {len(r_masked)} rows for {nu} users")
            rm = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in r_masked]) if nu else np.zeros(0),
                                      np.float32)
        pk = pen = None
        if rerank:
            pk = np.ascontiguousarray(partialk, np.int32).reshape(-1)
            pen = np.ascontiguousarray(penalties, np.float32).reshape(-1)
            if pk.size != ng or pen.size != 4 * ng:
                raise ValueError(f"partialk and penalties need {ng} entries and {ng} x 4 values")
        h = None
        if histories is not None:
            if len(histories) != nu:
                raise ValueError(f"histories has {len(histories)} lists for {nu} users")
            h = triples_csr(histories, 3)
        rin = None
        if scores is not None:
            rin = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in scores]), np.float32)
            if rin.size != N:
                raise ValueError(f"scores hold {rin.size} values for {N} candidates")
        rc = None if retrieval_coef is None else np.array([float(np.asarray(retrieval_coef).reshape(-1)[0])], np.float32)
        kc = None if rating_coefs is None else np.ascontiguousarray(np.asarray(rating_coefs, np.float32).reshape(-1)[:2])
        ids = np.empty(max(N, 1), np.int32) if rerank else None
        rout = np.empty(max(N, 1), np.float32)
        ptr = lambda a: None if a is None else a.ctypes.data
        hp = (None,) * 4 if h is None else tuple(ptr(a) for a in h)
        self._weights_before(user_weights, None)
        check(lib().rsys_rank_request(self._h, int(medium), ng, off.ctypes.data, ids_in.ctypes.data, ptr(pk), ptr(pen), ptr(q), nu, ptr(gp),
                                      ptr(rm), 0 if rm is None else rm.size, *hp, ptr(rc), ptr(kc), float(rating_mean), ptr(rin), ptr(ids),
                                      rout.ctypes.data))
        picked = None
        if rerank:
            picked = [ids[off[j]:off[j] + min(int(pk[j]), int(off[j + 1] - off[j]))].copy() for j in range(ng)]
        return picked, [rout[off[j]:off[j + 1]].copy() for j in range(ng)]

    # ---- a page from raw histories in one device pipeline (rsys_render_request: compute.jl:512-531 + render.jl:437-474)
    @staticmethod
    def _c_rows(d, rows, width):
        """an rsys_batch of `rows` rows of `width` columns holding the ten inference arrays only (+ the arrays it points into)"""
        b = _lib.rsys_batch()
        b.rows = rows
        keep = []

        def arr(x, dt):
            a = np.ascontiguousarray(np.asarray(x).reshape(-1), dt)
            if a.size != rows * width:
                raise ValueError(f"render_request: an array holds {a.size} values, expected {rows} x {width}")
            keep.append(a)
            return a.ctypes.data if a.size else None

        b.userid = arr(d["userid"], np.int32); b.token_mask_ids = arr(d["token_mask_ids"], np.int32)
        b.gender = arr(d["gender"], np.int32); b.source = arr(d["source"], np.int32)
        b.matchedid = arr(d["matchedid"], np.int32); b.status = arr(d["status"], np.int32)
        b.time = arr(d["time"], np.float64); b.rating = arr(d["rating"], np.float32); b.progress = arr(d["progress"], np.float32)
        b.rope_input_pos = arr(d["rope_input_pos"], np.int32)
        return b, keep

    def render_request(self, group_medium, offsets, limits, penalties, group, retrieval_rows, retrieval_token, ranking_prefix, prefix_stride,
                       user_desc, user_ts, adapter_slots=None, histories=None, selected=None, coef_have=None, coefs=None,
                       user_weights=None, selected_weights=None):
        """rsys_render_request: per group (medium, offset, limit, penalties (4)); per user its group, its row of `retrieval_rows` (the
        dict `serve.build_batch(..., "retrieval")` builds, n_users rows) with its query token `retrieval_token`, its row of
        `ranking_prefix` (the same ten arrays, `prefix_stride` columns per row), `user_desc` (nh, userid, gender, source) and `user_ts`;
        `adapter_slots` the bank slots of (0.retrieval, 0.ranking, 1.retrieval, 1.ranking) or None (base model); `histories` per user
        and `selected` per group as `retrieve_request` takes them; `coef_have` (2,) / `coefs` (2, 4) the registry's coefficients;
        `user_weights` / `selected_weights` as `retrieve_request` (they reach the retrieval and the ranking stage).
        Returns (one int32 page array per group, totals (n_groups,) int32)."""
        return self._render_call(False, group_medium, offsets, limits, penalties, group, retrieval_rows, retrieval_token, ranking_prefix,
                                 prefix_stride, user_desc, user_ts, adapter_slots, histories, selected, coef_have, coefs, user_weights,
                                 selected_weights)

    def render_request_full(self, group_medium, offsets, limits, penalties, group, retrieval_rows, retrieval_token, user_desc, user_ts,
                            adapter_slots=None, histories=None, selected=None, coef_have=None, coefs=None, user_weights=None,
                            selected_weights=None):
        """rsys_render_request_full: `render_request` with the ranking forward on full-length histories through the per-user K/V cache
        (DESIGN.md 4w).  The same arguments without `ranking_prefix` / `prefix_stride`; `user_desc` = (n_hist, userid, gender, source)
        with n_hist in [0, S - 1] = the history columns of the user's retrieval row (`serve.render_pack(..., full_history=True)`).  The
        library reserves max_rows cache slots when the model's reserve is smaller than a wave's users."""
        out = self._render_call(True, group_medium, offsets, limits, penalties, group, retrieval_rows, retrieval_token, None, 0, user_desc,
                                user_ts, adapter_slots, histories, selected, coef_have, coefs, user_weights, selected_weights)
        with_hist = int((np.asarray(user_desc, np.int32).reshape(-1, 4)[:, 0] >= 1).sum())
        if getattr(self, "rank_cache_slots", 0) < min(self.max_rows, with_hist):       # (the library reserved max_rows slots)
            self.rank_cache_slots = self.max_rows
        return out

    def _render_call(self, full, group_medium, offsets, limits, penalties, group, retrieval_rows, retrieval_token, ranking_prefix, prefix_stride,
                     user_desc, user_ts, adapter_slots, histories, selected, coef_have, coefs, user_weights=None, selected_weights=None):
        gm = np.ascontiguousarray(group_medium, np.int32).reshape(-1)
        ng = gm.size
        off = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        lim = np.ascontiguousarray(limits, np.int32).reshape(-1)
        pen = np.ascontiguousarray(penalties, np.float32).reshape(-1)
        gp = np.ascontiguousarray(group, np.int32).reshape(-1)
        nu = gp.size
        if off.size != ng or lim.size != ng or pen.size != 4 * ng:
            raise ValueError(f"render_request: offsets, limits and penalties need {ng} entries and {ng} x 4 values")
        S = self.config["max_sequence_length"]
        rb, keep_r = self._c_rows(retrieval_rows, nu, S)
        if not full:
            pb, keep_p = self._c_rows(ranking_prefix, nu, int(prefix_stride))
        tok = np.ascontiguousarray(retrieval_token, np.int32).reshape(-1)
        desc = np.ascontiguousarray(user_desc, np.int32).reshape(-1)
        ts = np.ascontiguousarray(user_ts, np.float64).reshape(-1)
        if tok.size != nu or desc.size != 4 * nu or ts.size != nu:
            raise ValueError(f"render_request: retrieval_token, user_desc and user_ts need {nu} entries ({nu} x 4 for user_desc)")
        sl = None if adapter_slots is None else np.ascontiguousarray(adapter_slots, np.int32).reshape(-1)
        if sl is not None and sl.size != 4:
            raise ValueError("render_request: adapter_slots holds the slots of 0.retrieval, 0.ranking, 1.retrieval, 1.ranking")
        h = None
        if histories is not None:
            if len(histories) != nu:
                raise ValueError(f"histories has {len(histories)} lists for {nu} users")
            h = triples_csr(histories, 3)
        sel = None
        if selected is not None:
            if len(selected) != ng:
                raise ValueError(f"selected has {len(selected)} lists for {ng} groups")
            sel = triples_csr(selected, 2)
        ch = None if coef_have is None else np.ascontiguousarray(coef_have, np.int32).reshape(-1)
        cf = None if coefs is None else np.ascontiguousarray(coefs, np.float32).reshape(-1)
        if (ch is not None and ch.size != 2) or (cf is not None and cf.size != 8):
            raise ValueError("render_request: coef_have holds 2 flags and coefs 2 x 4 values")
        cap = int(np.clip(lim, 0, None).sum())
        ids = np.empty(max(cap, 1), np.int32)
        ioff = np.empty(ng + 1, np.int64)
        total = np.empty(max(ng, 1), np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data
        hp = (None,) * 4 if h is None else tuple(ptr(a) for a in h)
        sp = (None,) * 3 if sel is None else tuple(ptr(a) for a in sel)
        prefix = () if full else (C.byref(pb), int(prefix_stride))
        fn = lib().rsys_render_request_full if full else lib().rsys_render_request
        self._weights_before(user_weights, selected_weights)
        check(fn(self._h, ng, ptr(gm), ptr(off), ptr(lim), ptr(pen), nu, ptr(gp), C.byref(rb), ptr(tok), *prefix, ptr(desc), ptr(ts), ptr(sl),
                 *hp, *sp, ptr(ch), ptr(cf), ptr(ids), cap, ptr(ioff), ptr(total)))
        return [ids[ioff[g]:ioff[g + 1]].copy() for g in range(ng)], total[:ng].copy()

    _RENDER_KEPT = {"time": np.float64, "rating": np.float32, "progress": np.float32, "queries": np.float32, "r_masked": np.float32,
                    "r": np.float32}

    def render_keep(self, on=True):
        """rsys_render_debug_keep (test hook): the following render_request calls keep their intermediates for render_kept"""
        check(lib().rsys_render_debug_keep(self._h, 1 if on else 0))

    def render_kept(self, key):
        """rsys_render_debug_get (test hook): the array the last render_request kept under `key` (flat; float32 / float64 / int32 by key)"""
        n = C.c_int64()
        check(lib().rsys_render_debug_get(self._h, key.encode(), None, 0, C.byref(n)))
        out = np.empty(n.value, np.uint8)
        check(lib().rsys_render_debug_get(self._h, key.encode(), out.ctypes.data, n.value, C.byref(n)))
        return out.view(self._RENDER_KEPT.get(key.split(".")[-1], np.int32))

    def rank_gram(self, medium, candidates):
        """rsys_rank_gram_get (test hook): per group the fp32 Gram matrix (n, n) of the candidates' item-similarity rows, as the
        reranking loop reads it."""
        cand = [np.asarray(c, np.int64).reshape(-1) for c in candidates]
        off = np.zeros(len(cand) + 1, np.int64)
        off[1:] = np.cumsum([c.size for c in cand])
        ids_in = np.ascontiguousarray(np.concatenate(cand), np.int32)
        n2 = int(sum(c.size * c.size for c in cand))
        out = np.empty(max(n2, 1), np.float32)
        check(lib().rsys_rank_gram_get(self._h, int(medium), len(cand), off.ctypes.data, ids_in.ctypes.data, out.ctypes.data, n2))
        res, at = [], 0
        for c in cand:
            res.append(out[at:at + c.size * c.size].reshape(c.size, c.size).copy()); at += c.size * c.size
        return res

    def trunk_output(self, rows):
        S = self.config["max_sequence_length"]; D = self.config["embed_dim"]
        out = np.empty((rows, 2 * S, D), np.float32)
        check(lib().rsys_trunk_output_get(self._h, out.ctypes.data, out.size))
        return out

    def debug_get(self, key, rows):
        """Bit-exact read-back of an index-path array of the last forward (rsys_debug_get; parity tests)."""
        S = self.batch_row_length or self.config["max_sequence_length"]; D = self.config["embed_dim"]; n = rows * S   # (a trimmed batch: its own row length)
        V = self.config["vocab_sizes"]["0_matchedid"] + self.config["vocab_sizes"]["1_matchedid"]
        if key == "forward.tokens":
            out = np.empty(1, np.int64)
        elif key == "npos":
            out = np.empty(4, np.int32)
        elif key in ("top.n", "top.cap", "infer.top", "infer.top_rows"):
            out = np.empty(1, np.int32)
        elif key == "host_syncs":
            out = np.empty(2, np.int32)
        elif key == "top.sel":
            out = np.empty(int(self.debug_get("top.cap", rows)[0]), np.int32)
        elif key == "top.slot":
            out = np.empty(2 * n, np.int32)
        elif key.startswith("idx."):
            out = np.empty(self.config["mask_topk"] * rows, np.int32)
        elif key.startswith("tokens."):
            out = np.empty(2 * n, np.int32)
        elif key == "embed.x0":
            out = np.empty((2 * n, D), np.float32)
        elif key.startswith("act."):     # act.<layer>.<x|xn|qkv|O|h|hn|ab|g>: saved activations (bf16 ones come back widened to float32)
            f = key.split(".")[2]
            H, KV = self.config["num_heads"], self.config["num_kv_heads"]
            Ip = (self.config["intermediate_dim"] + 127) // 128 * 128 if self.dtype in ("fp8", "float8") else (self.config["intermediate_dim"] + 15) // 16 * 16
            cols = {"x": D, "h": D, "xn": D, "hn": D, "O": D, "qkv": (H + 2 * KV) * (D // H), "ab": 2 * Ip, "g": Ip}[f]
            wide = f in ("x", "h") or self.dtype in ("fp32", "float32", "f32")
            out = np.empty((2 * n, cols), np.float32 if wide else np.uint16)
            check(lib().rsys_debug_get(self._h, key.encode(), out.ctypes.data, out.nbytes))
            return out if wide else (out.astype(np.uint32) << 16).view(np.float32)
        elif key.startswith("dw.") or key.startswith("f8keep."):   # bf16 operands the backward kept (widened to float32)
            f = key.split(".")[2]
            H, KV = self.config["num_heads"], self.config["num_kv_heads"]
            Ip = (self.config["intermediate_dim"] + 127) // 128 * 128 if self.dtype in ("fp8", "float8") else (self.config["intermediate_dim"] + 15) // 16 * 16
            cols = {"gxt": D, "dht": D, "dab": 2 * Ip, "dqkv": (H + 2 * KV) * (D // H)}.get(f, D)
            out = np.empty((2 * n, cols), np.uint16)
            check(lib().rsys_debug_get(self._h, key.encode(), out.ctypes.data, out.nbytes))
            return (out.astype(np.uint32) << 16).view(np.float32)
        elif key.startswith("f8."):
            L = self.config["num_layers"]
            out = np.empty({"f8.aamax": (L, 64, 32), "f8.wamax": (L, 8), "f8.desc": (L, 8, 32)}[key], np.float32)   # (aamax: [layer][shard][slot], take the max over the shards)
        elif key == "table.fused":
            out = np.empty((V + 1, D), np.float32)
        else:
            is_f32 = key in ("masked.rating", "masked.progress") or key.endswith(".label") or key.endswith(".weight")
            out = np.empty(n, np.float32 if is_f32 else np.int32)
        check(lib().rsys_debug_get(self._h, key.encode(), out.ctypes.data, out.nbytes))
        return out

    @property
    def forward_tokens(self):
        """tokens the last trunk forward ran over (rsys_debug_get "forward.tokens"): rows * 2 * the resident batch's row length"""
        return int(self.debug_get("forward.tokens", 0)[0])

    def param_checksum(self):
        """[fp64 sum, fp64 sum of squares, low / high 32 bits of a position-weighted integer sum of the bit patterns] of this rank's flat
        parameter buffer (a row-sharded model: without its own table rows), computed on the device in a fixed order: what the ranks
        compare instead of DDP's parameter broadcast (transformer.py:678-682; dist.assert_replicas_equal)"""
        out = (C.c_double * 4)()
        check(lib().rsys_param_checksum(self._h, C.byref(out)))
        return [float(x) for x in out]

    def head_rows(self):
        """positive-weight positions per task in the last forward (the head GEMMs stop there)."""
        out = (C.c_int32 * 4)()
        check(lib().rsys_head_rows_get(self._h, C.byref(out)))
        return [int(x) for x in out]

    # ---- instrumentation
    def timing(self, enable, serialize=False):
        """HIP-event timing of every kernel call site.  serialize no longer changes anything: it pulled the GEMMs of the
        side stream in line, and that stream is gone -- every kernel of the step runs on one stream (the argument stays for
        the callers that pass it)."""
        check(lib().rsys_op_timing(self._h, (2 if serialize else 1) if enable else 0))

    def timing_pause(self):
        """stop recording call-site events without waiting for the device; timing_report() later returns what was recorded"""
        check(lib().rsys_op_timing(self._h, 3))

    def timing_filter(self, substr):
        """time only the call sites whose name contains `substr` ("" = all); call after timing(True); cleared by timing(False)"""
        check(lib().rsys_op_timing_filter(self._h, (substr or "").encode()))

    def step_mark(self):
        """record a step boundary on the model's stream (no host sync)"""
        check(lib().rsys_step_mark(self._h))

    def step_times_ms(self, cap=65536):
        """milliseconds between consecutive step_mark() calls since the last read (synchronises)"""
        out = np.empty(cap, np.float32); n = C.c_int32()
        check(lib().rsys_step_marks_get(self._h, out.ctypes.data, cap, C.byref(n)))
        return out[: n.value].astype(np.float64)

    def timing_report(self):
        buf = C.create_string_buffer(1 << 16)
        check(lib().rsys_timing_get(self._h, buf, 1 << 16))
        rep = {}
        for line in buf.value.decode().splitlines():
            name, ms, cnt, fl = line.split()
            rep[name] = {"ms": float(ms), "count": int(cnt), "flops": float(fl)}
        return rep


def query_weights_array(weights):
    """flat contiguous float32 copy of query weights; a NaN or infinite weight raises (the library refuses it too)"""
    w = np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
    if not np.isfinite(w).all():
        raise ValueError("query weights must be finite")
    return w


def exclusion_csr(exclude, n_groups):
    """(offsets int64 [n_groups + 1], ids int32) of a list of per-group id arrays (ragged; duplicates allowed)."""
    if len(exclude) != n_groups:
        raise ValueError(f"exclude has {len(exclude)} lists for {n_groups} groups")
    parts = [np.asarray(e, np.int64).reshape(-1) for e in exclude]
    off = np.zeros(n_groups + 1, np.int64)
    off[1:] = np.cumsum([p.size for p in parts])
    ids = np.concatenate(parts).astype(np.int32) if parts and off[-1] else np.zeros(1, np.int32)
    return off, np.ascontiguousarray(ids)


def csc_parts(a):
    """(indptr int64, indices int32, data float32, shape) of a 0-based CSC matrix given as an (indptr, indices, data, shape) tuple or
    an object with those attributes (a scipy CSC matrix; scipy itself is not needed)."""
    if isinstance(a, (tuple, list)):
        indptr, indices, data, shape = a
    else:
        indptr, indices, data, shape = a.indptr, a.indices, a.data, a.shape
    indptr = np.ascontiguousarray(indptr, np.int64).reshape(-1)
    indices = np.ascontiguousarray(indices, np.int32).reshape(-1)
    data = np.ascontiguousarray(data, np.float32).reshape(-1)
    shape = tuple(int(x) for x in shape)
    if len(shape) != 2 or indptr.size != shape[1] + 1:
        raise ValueError(f"CSC indptr has {indptr.size} entries for shape {shape}")
    if indices.size != data.size or indptr[-1] > indices.size:
        raise ValueError("CSC indices and data must hold indptr[-1] entries")
    return indptr, np.ascontiguousarray(indices[:max(int(indptr[-1]), 0)]), np.ascontiguousarray(data[:max(int(indptr[-1]), 0)]), shape


def triples_csr(lists, width):
    """(offsets int64 [n + 1], then `width` int32 columns) of a list of per-row sequences of `width`-tuples (ragged; order kept)."""
    lens = [len(x) for x in lists]
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    if n == 0:
        flat = np.zeros((1, width), np.int64)
    elif all(isinstance(x, np.ndarray) for x in lists):
        flat = np.concatenate([np.asarray(x, np.int64).reshape(-1, width) for x in lists])
    else:   # (one pass over the Python tuples: a request's lists hold tens of thousands of them)
        flat = np.fromiter(itertools.chain.from_iterable(itertools.chain.from_iterable(lists)), np.int64, count=n * width).reshape(n, width)
    return (off,) + tuple(np.ascontiguousarray(flat[:, j], np.int32) for j in range(width))


def gather_rows(host_group, rows):
    """the ranks' row blocks of a row-sharded table, concatenated in rank order (over the TCP control plane)"""
    rows = np.ascontiguousarray(rows, np.float32)
    parts = host_group.all_gather_bytes(rows.tobytes())
    return np.concatenate([np.frombuffer(b, np.float32).reshape(-1, rows.shape[1]) for b in parts], axis=0)


def synchronize():
    check(lib().rsys_device_synchronize())
