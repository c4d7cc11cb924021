"""The search model (Training/search/train.py) on the device, under the reference's names: text-query embeddings
(Import/embeddings/embed_queries.jl, 3072 wide) are matched against the transformer's item table of one medium (`masked.{m}`, 2048 wide)
through one trainable linear map and a logit scale.

The device work goes through the rsys_search_* entry points of include/rsys.h: forward, soft-max loss and backward in the factored order
(the [V][Q] matrix W = E Wenc^T is never formed in training), AdamW with the GradScaler skip rule, the export `search.{m}` and a top-k
serving call.  This module holds the dataset, the training loop, early stopping, checkpoints and the export files.  Inputs are plain
arrays, `.npz` chunk files, or `.h5` chunk files where the package's HDF5 adapter is built."""
import ctypes as C
import glob
import os

import numpy as np

from ._encoder_handle import EarlyStopper, EncoderHandle, _ptr, load_checkpoint, write_checkpoint  # noqa: F401 (re-exported)
from ._lib import check, lib

DTYPES = {"fp32": 0, "bf16": 1}
CHUNK_KEYS = ("queries", "matchedids", "mediums", "counts")


def training_config(vocab_sizes, learning_rate=3e-4, batch_size=1024, embed_dim=2048, query_dim=3072):
    """train.py:282-288; embed_dim / query_dim are the widths the reference hard-codes (train.py:81,86)"""
    return {"vocab_sizes": dict(vocab_sizes), "learning_rate": learning_rate, "batch_size": batch_size, "embed_dim": embed_dim,
            "query_dim": query_dim}


def read_chunk(fn):
    """one {split}.{i} chunk file: .npz, or .h5 through the package's adapter"""
    if fn.endswith(".npz"):
        with np.load(fn) as z:
            return {k: z[k] for k in z.files}
    from . import h5
    if not os.path.exists(h5.LIB_PATH):
        raise RuntimeError(f"{fn}: the HDF5 adapter (librsys_h5.so) is not built here; convert the chunk to .npz")
    return h5.read_h5(fn)


class SearchDataset:
    """SearchDataset (train.py:16-54) for one medium: chunks are files `{datadir}/{datasplit}.*.h5` / `.npz` or in-memory dicts with
    the keys queries [N][Q], matchedids [N], mediums [N], counts [N].  Per chunk: rows of the other medium dropped, weight =
    sqrt(counts); when shuffling, the chunk order and the row order are shuffled and the rows padded to a multiple of batch_size by
    np.random.choice over the indices collected so far; otherwise the last batch is ragged.  The randomness comes from a seedable
    Generator (the reference uses numpy's global one)."""

    def __init__(self, datasplit, batch_size, shuffle, medium, datadir=None, chunks=None, seed=0):
        assert (datadir is None) != (chunks is None), "give datadir or chunks"
        assert batch_size >= 1
        self.datasplit = datasplit
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.medium = medium
        if chunks is None:
            self.chunks = sorted(glob.glob(os.path.join(datadir, f"{datasplit}.*.h5")) + glob.glob(os.path.join(datadir, f"{datasplit}.*.npz")))
        else:
            self.chunks = list(chunks)
        for c in self.chunks:
            if not isinstance(c, str):
                missing = [k for k in CHUNK_KEYS if k not in c]
                if missing:
                    raise ValueError(f"SearchDataset: chunk without {missing}")
        self.rng = np.random.default_rng(seed)

    def __iter__(self):
        order = list(range(len(self.chunks)))
        if self.shuffle:
            self.rng.shuffle(order)
        for ci in order:
            c = self.chunks[ci]
            d = read_chunk(c) if isinstance(c, str) else c
            d = {k: np.asarray(d[k]) for k in CHUNK_KEYS}
            mask = d["mediums"] == self.medium
            d = {k: v[mask] for k, v in d.items()}
            d["weight"] = np.sqrt(d["counts"].astype(np.float64))
            del d["counts"]
            idxs = list(range(len(d["matchedids"])))
            if not idxs:
                continue
            if self.shuffle:
                self.rng.shuffle(idxs)
                while len(idxs) % self.batch_size != 0:
                    idxs.append(int(self.rng.choice(idxs)))
            for i in range(0, len(idxs), self.batch_size):
                idx = idxs[i:i + self.batch_size]
                yield {k: v[idx, ...] for k, v in d.items()}


class SearchModel(EncoderHandle):
    """SearchModel (train.py:76-130) of one medium over an rsys_search handle.  features: the frozen table E_m [V_m][D] (the medium's
    rows of `retrieval_embeddings.weight`), or a RecommenderModel whose item table of `medium` is copied on the device
    (rsys_search_features_from_model: no host round trip)."""

    _PREFIX = "rsys_search"

    def __init__(self, config, medium, features, dtype="bf16", max_batch=None, device=0):
        if dtype not in DTYPES:
            raise ValueError(f"SearchModel: dtype must be one of {sorted(DTYPES)}")
        if medium not in config["vocab_sizes"]:
            raise ValueError(f"SearchModel: medium {medium} is not in vocab_sizes")
        self.config = config
        self.medium = medium
        self.V = int(config["vocab_sizes"][medium])
        self.D = int(config.get("embed_dim", 2048))
        self.Q = int(config.get("query_dim", 3072))
        self.max_batch = int(max_batch or config["batch_size"])
        source_model = features if hasattr(features, "item_embeddings") else None
        if source_model is None:
            f = np.ascontiguousarray(features, np.float32)
            if f.shape != (self.V, self.D):
                raise ValueError(f"SearchModel: features are {f.shape}, the config says ({self.V}, {self.D})")
        if self.D % 64 or self.Q % 64:
            raise ValueError("SearchModel: embed_dim and query_dim must be multiples of 64")
        if not 1 <= self.max_batch <= 4096:
            raise ValueError("SearchModel: 1 <= max_batch <= 4096")
        self.dtype = dtype
        self.h = None
        h = C.c_void_p()
        check(lib().rsys_search_create(self.V, self.D, self.Q, DTYPES[dtype], self.max_batch, device, C.byref(h)))
        self.h = h
        if source_model is not None:
            check(lib().rsys_search_features_from_model(self.h, source_model._h, medium))
        else:
            check(lib().rsys_search_features_set(self.h, _ptr(f), self.V, self.D))
        self.training = True
        self.has_optimizer = False

    def _tensor(self, name):
        if name not in ("encoder.weight", "logit_scale"):
            raise KeyError(f"SearchModel: unknown parameter {name!r} (encoder.weight, logit_scale)")
        return (self.Q, self.D) if name == "encoder.weight" else ()

    def init_weights(self, seed=0):
        """nn.Linear's default init of the encoder: U(-1 / sqrt(D), 1 / sqrt(D)); logit_scale = 1"""
        b = 1.0 / np.sqrt(self.D)
        self.param_set("encoder.weight", np.random.default_rng(seed).uniform(-b, b, (self.Q, self.D)))
        self.param_set("logit_scale", 1.0)

    def state_dict(self):
        return {"logit_scale": self.param_get("logit_scale"), "encoder.weight": self.param_get("encoder.weight")}

    def load_state_dict(self, d):
        for name in ("logit_scale", "encoder.weight"):
            self.param_set(name, d[name])

    def _batch(self, batch):
        x = np.ascontiguousarray(batch["queries"], np.float32)
        y = np.ascontiguousarray(batch["matchedids"], np.int32).reshape(-1)
        w = np.ascontiguousarray(np.asarray(batch["weight"]).reshape(-1), np.float32)
        if x.ndim != 2 or x.shape[1] != self.Q:
            raise ValueError(f"SearchModel: queries must be [B][{self.Q}]")
        if not (len(y) == len(w) == x.shape[0]):
            raise ValueError("SearchModel: queries, matchedids and weight disagree on the batch size")
        if "mediums" in batch and np.any(np.asarray(batch["mediums"]) != self.medium):
            raise ValueError(f"SearchModel: the batch holds rows of another medium than {self.medium}")
        return x, y, w

    def forward_backward(self, batch, evaluate=False):
        """model(d) (+ loss.backward() unless evaluate): returns (loss, raw weight sum)"""
        x, y, w = self._batch(batch)
        if not 1 <= len(y) <= self.max_batch:
            raise ValueError(f"SearchModel: 1 <= B <= {self.max_batch}")
        loss, wsum = C.c_float(0), C.c_float(0)
        check(lib().rsys_search_forward_backward(self.h, _ptr(x), _ptr(y), _ptr(w), len(y), 1 if evaluate else 0, C.byref(loss),
                                                 C.byref(wsum)))
        return loss.value, wsum.value

    def create_optimizer(self, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1):
        check(lib().rsys_search_adamw_create(self.h, betas[0], betas[1], eps, weight_decay))
        self.has_optimizer = True

    def adamw_state_set(self, name, exp_avg, exp_avg_sq, step):
        m = np.ascontiguousarray(np.asarray(exp_avg, np.float32).reshape(self._tensor(name)))
        v = np.ascontiguousarray(np.asarray(exp_avg_sq, np.float32).reshape(self._tensor(name)))
        check(lib().rsys_search_adamw_state_set(self.h, name.encode(), _ptr(m), _ptr(v), m.size, int(step)))

    def embed(self):
        """SearchModel.embed restricted to the medium: E_m Wenc^T, fp32 [V_m][Q]"""
        out = np.zeros((self.V, self.Q), np.float32)
        check(lib().rsys_search_export(self.h, _ptr(out)))
        return out

    def topk(self, queries, k):
        """per query the k most probable items of the medium: (ids int32 [n][k], log-probabilities f32 [n][k]), ties by ascending id"""
        x = np.ascontiguousarray(queries, np.float32)
        if x.ndim != 2 or x.shape[1] != self.Q:
            raise ValueError(f"SearchModel: queries must be [n][{self.Q}]")
        if not 1 <= x.shape[0] <= self.max_batch:
            raise ValueError(f"SearchModel: 1 <= n_queries <= {self.max_batch}")
        if not 1 <= k <= min(self.V, 8192):
            raise ValueError("SearchModel: 1 <= k <= min(V_m, 8192)")
        ids = np.zeros((x.shape[0], k), np.int32)
        lp = np.zeros((x.shape[0], k), np.float32)
        check(lib().rsys_search_topk(self.h, _ptr(x), x.shape[0], k, _ptr(ids), _ptr(lp)))
        return ids, lp

    def text_rows(self, queries):
        """rsys_op_text_rows: what rsys_query_texts_set computes for a request's text queries, to the host -- the logits
        z (n, V_m) float32 of n <= min(64, max_batch) query embeddings over the medium's items and their log-sum-exp (n,); z - lse[:, None]
        is `topk`'s log-probability per id, scored by the streaming kernel instead of the 256-row GEMM"""
        x = np.ascontiguousarray(queries, np.float32)
        if x.ndim != 2 or x.shape[1] != self.Q:
            raise ValueError(f"SearchModel: queries must be [n][{self.Q}]")
        z = np.zeros((x.shape[0], self.V), np.float32)
        lse = np.zeros(x.shape[0], np.float32)
        check(lib().rsys_op_text_rows(self.h, _ptr(x), x.shape[0], _ptr(z), _ptr(lse)))
        return z, lse

    def debug(self, name, shape):
        out = np.zeros(shape, np.float32)
        check(lib().rsys_search_debug_get(self.h, name.encode(), _ptr(out), out.size))
        return out


def create_optimizer(model, config=None):
    """train.py:181-192: AdamW with torch's default betas and eps, weight decay 0.1 on the matrix and 0 on the scalar"""
    model.create_optimizer()
    return model


class ConstantScheduler:
    """train.py:195-201"""

    def __init__(self):
        self.steps = 0

    def __call__(self, epoch):
        self.steps += 1
        return 1


def evaluate_metrics(model, dataset):
    """train.py:133-149: sum loss * (raw sum w) / sum (raw sum w) over the split, forward only"""
    losses = weights = 0.0
    model.eval()
    for b in dataset:
        loss, w = model.forward_backward(b, evaluate=True)
        losses += loss * w
        weights += w
    model.train()
    return losses / weights if weights != 0 else float("nan")


def train_epoch(model, dataset, scheduler=None, lr=None):
    """train.py:152-178: per batch zero_grad, forward + backward, clip 1.0, AdamW (skipped on a non-finite gradient), scheduler step"""
    lr = model.config["learning_rate"] if lr is None else lr
    losses = weights = 0.0
    for step, b in enumerate(dataset):
        model.zero_grad()
        loss, w = model.forward_backward(b)
        losses += loss * w
        weights += w
        factor = scheduler(step) if scheduler is not None else 1
        model.adamw_step(lr * factor, 1.0)
    return losses / weights if weights != 0 else float("nan")


def checkpoint_model(model, epoch, training_loss, test_loss, save, datadir, medium=None):
    """train.py:248-272: search.model.{m}.npz under the reference's state-dict names (+ epoch and losses) when `save`, and a row of
    search.model.{m}.csv (header written at epoch -1)"""
    write_checkpoint("search.model", model, epoch, training_loss, test_loss, save, datadir, model.medium if medium is None else medium)


def train(model, training, test, datadir, num_epochs=1024, log=print):
    """train.py:291-343: the epoch -1 test evaluation (training loss inf), then per epoch train_epoch, the test evaluation, early
    stopping (patience 5, rtol 1e-3) and checkpoints.  training / test: SearchDatasets of the model's medium.  Returns the best
    (training, test) losses; the best parameters are in search.model.{m}.npz."""
    if not model.has_optimizer:
        create_optimizer(model)
    scheduler = ConstantScheduler()
    stopper = EarlyStopper(patience=5, rtol=0.001)
    training_loss = float("inf")
    test_loss = evaluate_metrics(model, test)
    log(f"Epoch: -1, Test Loss: {test_loss}")
    stopper(test_loss)
    checkpoint_model(model, -1, training_loss, test_loss, True, datadir)
    best = (training_loss, test_loss)
    for epoch in range(num_epochs):
        training_loss = train_epoch(model, training, scheduler)
        log(f"Epoch: {epoch}, Training Loss: {training_loss}")
        test_loss = evaluate_metrics(model, test)
        log(f"Epoch: {epoch}, Test Loss: {test_loss}")
        stopper(test_loss)
        if stopper.save_model:
            best = (training_loss, test_loss)
        checkpoint_model(model, epoch, training_loss, test_loss, stopper.save_model, datadir)
        if stopper.stop:
            break
    log(f"Best losses: {best}")
    return best


def generate_embeddings(model, datadir=None):
    """train.py:346-371: {"search.{m}": E_m Wenc^T [V_m][Q] f32, "temperature": [logit_scale]} of the model as it stands (load the
    checkpoint first); written to output.embeddings.{m}.npz, and to .h5 where the HDF5 adapter is built, when datadir is given"""
    d = {f"search.{model.medium}": model.embed(), "temperature": np.array([model.get_temperature()], np.float64)}
    if datadir is not None:
        np.savez(os.path.join(datadir, f"output.embeddings.{model.medium}.npz"), **d)
        from . import h5
        if os.path.exists(h5.LIB_PATH):
            h5.write_h5(os.path.join(datadir, f"output.embeddings.{model.medium}.h5"), d)
    return d
