"""The item-similarity LambdaRank model (Training/item_similarity/pairwise_ltr.py, run by item_similarity/run.jl with --features transformer)
on the device, under the reference's names, and the cross-medium map of Finetune/pairwise.jl.

The device work goes through the rsys_sim_* entry points of include/rsys.h: forward, LambdaRank loss and backward, nDCG, AdamW, the
embedding export and the hard-negative mining.  This module holds the dataset assembly, the training loop, early stopping, checkpoints
and the tables `serve.load_retrieval_tables` reads.  Inputs are plain arrays: the columns of pairs.{m}.csv and the boolean testmask.

The acceptance metrics of Training/item_similarity/pairwise_metrics.jl (nDCG@k and Recall@k of every test target ranked against the whole
catalogue) are at the end of the file: the ranks come from rsys_sim_pair_ranks, the fp64 arithmetic is done here."""
import csv
import ctypes as C
import math
import os

import numpy as np

from ._encoder_handle import EarlyStopper, EncoderHandle, _ptr, load_checkpoint, write_checkpoint  # noqa: F401 (re-exported)
from ._lib import check, lib

DTYPES = {"fp32": 0, "bf16": 1}


def training_config(vocab_sizes, embed_dim=1024, learning_rate=3e-4, batch_size=128, items_per_query=2048):
    """pairwise_ltr.py:364-372"""
    return {"vocab_sizes": dict(vocab_sizes), "embed_dim": embed_dim, "learning_rate": learning_rate, "batch_size": batch_size,
            "items_per_query": items_per_query}


def read_pairs_csv(path):
    """pairs.{m}.csv as columns (stdlib csv): cliptype, source_matchedid, source_popularity, target_matchedid, score"""
    cols = {k: [] for k in ("cliptype", "source_matchedid", "source_popularity", "target_matchedid", "score")}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for k in cols:
                cols[k].append(row[k])
    try:
        clip = np.array([int(x) for x in cols["cliptype"]])
    except ValueError:
        clip = np.array(cols["cliptype"])
    return {"cliptype": clip, "source_matchedid": np.array(cols["source_matchedid"], np.int64),
            "source_popularity": np.array(cols["source_popularity"], np.float64),
            "target_matchedid": np.array(cols["target_matchedid"], np.int64), "score": np.array(cols["score"], np.float64)}


def pack_testmask(testmask):
    """bool [V][V] -> the bit rows of rsys_sim_testmask_set: int32 [V][ceil(V / 32)], bit j & 31 of word j >> 5 = testmask[i, j]"""
    m = np.asarray(testmask, bool)
    V = m.shape[0]
    W = (m.shape[1] + 31) // 32
    b = np.packbits(m, axis=1, bitorder="little")
    pad = np.zeros((V, 4 * W), np.uint8)
    pad[:, :b.shape[1]] = b
    return np.ascontiguousarray(pad).view("<u4").astype(np.uint32).view(np.int32).reshape(V, W)


class LTRModel(EncoderHandle):
    """LTRModel (pairwise_ltr.py:124-213) over an rsys_sim handle: `embed`, `process_batch`, `lambdarank_loss`, `ndcg` run on the
    device.  features: the frozen [V][F] table (F = 2048: transformer; 5120: [transformer | content]), or a RecommenderModel whose
    item table of `medium` is copied on the device (rsys_sim_features_from_model: no host round trip)."""

    _PREFIX = "rsys_sim"

    def __init__(self, config, medium, features, dtype="bf16", max_queries=None, dropout=0.1, device=0, content=None):
        self.config = config
        self.medium = medium
        source_model = features if hasattr(features, "item_embeddings") else None
        if source_model is not None:
            assert content is None, "the content table goes with host features"
            f = None
            self.transformer_embeddings = None
            self.content_embeddings = None
            self.V, self.F = config["vocab_sizes"][medium], source_model.config["embed_dim"]
        else:
            f = np.asarray(features, np.float32)
            self.transformer_embeddings = f
            self.content_embeddings = None if content is None else np.asarray(content, np.float32)
            if self.content_embeddings is not None:
                f = np.concatenate([f, self.content_embeddings], axis=1)
            self.V, self.F = f.shape
        self.E = config["embed_dim"]
        self.n = config["items_per_query"]
        self.dtype = dtype
        self.dropout = dropout
        h = C.c_void_p()
        check(lib().rsys_sim_create(self.V, self.F, self.E, DTYPES[dtype], max_queries or config["batch_size"], self.n, dropout, device,
                                    C.byref(h)))
        self.h = h
        if source_model is not None:
            check(lib().rsys_sim_features_from_model(self.h, source_model._h, medium))
        else:
            f = np.ascontiguousarray(f)
            check(lib().rsys_sim_features_set(self.h, _ptr(f), self.V, self.F))
        self.training = True
        self.seed = 0
        self.step = 0

    def _tensor(self, name):
        return (self.E, self.F) if name == "encoder.1.weight" else ()

    def state_dict(self):
        d = {"logit_scale": self.param_get("logit_scale"), "encoder.1.weight": self.param_get("encoder.1.weight")}
        if self.transformer_embeddings is not None:   # (features taken from a model on the device stay with that model)
            d["transformer_embeddings.weight"] = self.transformer_embeddings
        if self.content_embeddings is not None:
            d["content_embeddings.weight"] = self.content_embeddings
        return d

    def load_state_dict(self, d):
        for name in ("logit_scale", "encoder.1.weight"):
            self.param_set(name, d[name])

    @staticmethod
    def _batch(batch):
        src = np.ascontiguousarray(np.asarray(batch["sourceid"])[:, 0], np.int32)
        tgt = np.ascontiguousarray(batch["targetid"], np.int32)
        rel = np.ascontiguousarray(batch["relevance"], np.float32)
        w = np.ascontiguousarray(np.asarray(batch["weight"]).reshape(-1), np.float32)
        return src, tgt, rel, w

    def forward_backward(self, batch, evaluate=False, seed=None, step=None):
        """model(d) + loss.backward() (train_epoch, pairwise_ltr.py:244-252); returns the batch loss"""
        src, tgt, rel, w = self._batch(batch)
        loss = C.c_float(0)
        check(lib().rsys_sim_forward_backward(self.h, len(src), tgt.shape[1], _ptr(src), _ptr(tgt), _ptr(rel), _ptr(w),
                                              1 if evaluate else 0, self.seed if seed is None else seed,
                                              self.step if step is None else step, C.byref(loss)))
        return loss.value

    def ndcg(self, batch):
        """(sum w nDCG, sum w) of a batch in eval mode (pairwise_ltr.py:192-208)"""
        src, tgt, rel, w = self._batch(batch)
        out = (C.c_double * 2)()
        check(lib().rsys_sim_ndcg(self.h, len(src), tgt.shape[1], _ptr(src), _ptr(tgt), _ptr(rel), _ptr(w), C.byref(out)))
        return out[0], out[1]

    def embed_all(self, train_mode=None, seed=None):
        """every id embedded in fp32 [V][E]; held on the device for hard_negatives"""
        out = np.zeros((self.V, self.E), np.float32)
        tm = self.training if train_mode is None else train_mode
        check(lib().rsys_sim_embed_all(self.h, 1 if tm else 0, self.seed if seed is None else seed, _ptr(out)))
        return out

    def set_export(self, emb):
        e = np.ascontiguousarray(emb, np.float32)
        assert e.shape == (self.V, self.E)
        check(lib().rsys_sim_export_set(self.h, _ptr(e)))

    def set_testmask(self, testmask):
        bits = pack_testmask(testmask)
        check(lib().rsys_sim_testmask_set(self.h, _ptr(bits)))

    def hard_negatives(self, split, sources, positives, n):
        """load_hard_negatives' selection: [len(sources)][n] ids, ascending score (rsys_sim_hard_negatives)"""
        src = np.ascontiguousarray(sources, np.int32)
        off = np.zeros(len(src) + 1, np.int64)
        off[1:] = np.cumsum([len(p) for p in positives])
        pid = np.ascontiguousarray(np.concatenate([np.asarray(p, np.int32) for p in positives]) if len(positives) else
                                   np.zeros(0, np.int32), np.int32)
        out = np.zeros((len(src), n), np.int32)
        check(lib().rsys_sim_hard_negatives(self.h, 0 if split == "training" else 1, len(src), _ptr(src), _ptr(off),
                                            _ptr(pid) if pid.size else _ptr(np.zeros(1, np.int32)), n, _ptr(out)))
        return out

    @staticmethod
    def _csr(sources, targets):
        src = np.ascontiguousarray(sources, np.int32)
        assert len(targets) == len(src), "one target list per source"
        off = np.zeros(len(src) + 1, np.int64)
        off[1:] = np.cumsum([len(t) for t in targets])
        tid = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int32).reshape(-1) for t in targets]) if len(targets) else
                                   np.zeros(0, np.int32), np.int32)
        return src, off, tid

    def pair_ranks(self, sources, targets):
        """pairwise_metrics.jl's ranking (rsys_sim_pair_ranks): per source s the 1-based rank of each of its targets among all items
        i != s, by the held export's fp32 Gram row times the held testmask row, in sortperm(rev = true) order; 0 for a target equal to
        its source.  targets: one id sequence per source.  Returns one int32 array per source."""
        src, off, tid = self._csr(sources, targets)
        out = np.zeros(max(int(off[-1]), 1), np.int32)
        check(lib().rsys_sim_pair_ranks(self.h, len(src), _ptr(src), _ptr(off), _ptr(tid if tid.size else np.zeros(1, np.int32)), _ptr(out)))
        return [out[off[i]:off[i + 1]] for i in range(len(src))]

    def pair_scores(self, sources):
        """test hook: the masked score rows pair_ranks ranks, f32 [len(sources)][V] (rsys_sim_pair_scores)"""
        src = np.ascontiguousarray(sources, np.int32)
        out = np.zeros((len(src), self.V), np.float32)
        check(lib().rsys_sim_pair_scores(self.h, len(src), _ptr(src), _ptr(out)))
        return out

    def debug(self, name, shape, dtype):
        out = np.zeros(shape, dtype)
        check(lib().rsys_sim_debug_get(self.h, name.encode(), _ptr(out), out.size))
        return out


def group_queries(pairs, testmask, datasplit):
    """LTRDataset.load_queries (pairwise_ltr.py:31-54): one query per (cliptype, source, popularity) group in key order, its targets
    those with testmask[source, target] == (split is test), sorted by score descending (stable); empty queries dropped"""
    groups = {}
    for c, s, p, t, sc in zip(pairs["cliptype"], pairs["source_matchedid"], pairs["source_popularity"], pairs["target_matchedid"],
                              pairs["score"]):
        groups.setdefault((c.item() if hasattr(c, "item") else c, int(s), float(p)), []).append((int(t), float(sc)))
    queries = []
    for (c, s, p) in sorted(groups):
        targets = sorted([(t, sc) for (t, sc) in groups[(c, s, p)] if (datasplit == "test") == bool(testmask[s, t])],
                         key=lambda x: x[1], reverse=True)
        queries.append({"sourceid": s, "popularity": math.sqrt(p), "targets": targets})
    return [q for q in queries if q["targets"]]


class LTRDataset:
    """LTRDataset (pairwise_ltr.py:16-110): queries, positive caps (int(n * 0.9) in training, n in test), hard negatives mined on the
    device from the model's held export, lists of n = positives then negatives"""

    def __init__(self, datasplit, config, pairs, testmask, model=None):
        assert datasplit in ("training", "test")
        self.datasplit = datasplit
        self.config = config
        self.num_items_per_query = config["items_per_query"]
        self.max_num_positives = int(round(self.num_items_per_query) * 0.9) if datasplit == "training" else self.num_items_per_query
        self.queries = group_queries(pairs, testmask, datasplit)
        self.hard_negatives = {}
        if model is not None:
            self.load_hard_negatives(model)

    def load_hard_negatives(self, model):
        """scores against the model's held export (embed_all / set_export); the positives of the last query of a source are excluded,
        as the reference's dict `targets` keeps the last one"""
        targets = {q["sourceid"]: q["targets"] for q in self.queries}
        sources = list(dict.fromkeys(q["sourceid"] for q in self.queries))
        if not sources:
            return
        pos = [[t for t, _ in targets[s][:self.max_num_positives]] for s in sources]
        ids = model.hard_negatives(self.datasplit, sources, pos, self.num_items_per_query)
        self.hard_negatives = {s: ids[i] for i, s in enumerate(sources)}

    def __len__(self):
        return len(self.queries)

    def __getitem__(self, idx):
        q = self.queries[idx]
        pos = q["targets"][:self.max_num_positives]
        k = self.num_items_per_query - len(pos)
        neg = list(self.hard_negatives[q["sourceid"]][-k:]) if k > 0 else []
        return {"sourceid": np.full(self.num_items_per_query, q["sourceid"], np.int64),
                "targetid": np.array([t for t, _ in pos] + neg, np.int64),
                "relevance": np.array([r for _, r in pos] + [0.0] * k, np.float64),
                "weight": np.array([q["popularity"]], np.float64)}

    def batches(self, batch_size, shuffle=False, rng=None):
        order = np.arange(len(self))
        if shuffle:
            order = (rng or np.random.default_rng()).permutation(len(self))
        for i in range(0, len(order), batch_size):
            items = [self[j] for j in order[i:i + batch_size]]
            yield {k: np.stack([it[k] for it in items]) for k in items[0]}


def evaluate_metrics(model, dataset, batch_size=None):
    """1 - the w-weighted nDCG over the split (pairwise_ltr.py:215-231)"""
    model.eval()
    losses = weights = 0.0
    for b in dataset.batches(batch_size or model.config["batch_size"]):
        s, w = model.ndcg(b)
        losses += s
        weights += w
    model.train()
    return 1.0 - losses / weights if weights != 0 else float("nan")


def train_epoch(model, dataset, rng=None, lr=None):
    """pairwise_ltr.py:234-260: per batch zero_grad, forward + backward (every list slot its own dropout mask), clip 1.0, AdamW"""
    lr = model.config["learning_rate"] if lr is None else lr
    losses = weights = 0.0
    for b in dataset.batches(model.config["batch_size"], shuffle=True, rng=rng):
        model.zero_grad()
        loss = model.forward_backward(b)
        w = float(np.sum(b["weight"]))
        losses += loss * w
        weights += w
        model.adamw_step(lr, 1.0)
        model.step += 1
    return losses / weights


def checkpoint_model(model, epoch, training_loss, test_loss, save, datadir, medium):
    """pairwise_ltr.py:330-355: pairwise.model.{m}.npz under the reference's state-dict names (+ epoch and losses) when `save`, and a row
    of pairwise.model.{m}.csv (header written at epoch -1)"""
    write_checkpoint("pairwise.model", model, epoch, training_loss, test_loss, save, datadir, medium)


def generate_embeddings(model):
    """pairwise_ltr.py:450-472: (embeddings [V][E] fp32, temperature); in train mode the export carries dropout, as inside train()"""
    return model.embed_all(), model.get_temperature()


def train(model, pairs, testmask, datadir, num_epochs=1024, seed=0, log=print):
    """pairwise_ltr.py:375-436: initial export and hard negatives, the epoch -1 evaluation, then per epoch train_epoch, a train-mode
    export, re-mined hard negatives for both splits, evaluation, early stopping (patience 5, rtol 1e-3) and checkpoints.  Returns the
    best (training, test) losses; the best parameters are in pairwise.model.{m}.npz."""
    rng = np.random.default_rng(seed)
    model.seed = seed
    model.set_testmask(testmask)
    model.train()
    generate_embeddings(model)
    data = {x: LTRDataset(x, model.config, pairs, testmask, model) for x in ("training", "test")}
    stopper = EarlyStopper(patience=5, rtol=0.001)
    training_loss = evaluate_metrics(model, data["training"])
    test_loss = evaluate_metrics(model, data["test"])
    log(f"Epoch: -1, Training Loss: {training_loss}, Test Loss: {test_loss}")
    stopper(test_loss)
    checkpoint_model(model, -1, training_loss, test_loss, True, datadir, model.medium)
    best = (training_loss, test_loss)
    for epoch in range(num_epochs):
        train_epoch(model, data["training"], rng)
        model.seed = seed + epoch + 1
        generate_embeddings(model)
        for x in ("training", "test"):
            data[x].load_hard_negatives(model)
        training_loss = evaluate_metrics(model, data["training"])
        test_loss = evaluate_metrics(model, data["test"])
        log(f"Epoch: {epoch}, Training Loss: {training_loss}, Test Loss: {test_loss}")
        stopper(test_loss)
        if stopper.save_model:
            best = (training_loss, test_loss)
        checkpoint_model(model, epoch, training_loss, test_loss, stopper.save_model, datadir, model.medium)
        if stopper.stop:
            break
    return best


def closest_orthogonal_map(A, B):
    """Finetune/pairwise.jl:99-103 on Julia-shaped (dim x N) matrices: U V^T of svd(B A^T)"""
    U, _, Vt = np.linalg.svd(np.asarray(B, np.float64) @ np.asarray(A, np.float64).T)
    return U @ Vt


def avg_norm(x):
    """Finetune/pairwise.jl:105-107"""
    x = np.asarray(x, np.float64)
    return float(np.sum(x ** 2) / (x.shape[0] * x.shape[1]))


def cross_medium_map(emb_m, emb_o, source_ids, target_ids):
    """crossproject.{m}: the orthogonal map from medium m's embeddings ([V_m][E]) onto medium 1 - m's over the adaptation pairs"""
    A = np.asarray(emb_m, np.float64)[np.asarray(source_ids)].T
    B = np.asarray(emb_o, np.float64)[np.asarray(target_ids)].T
    return closest_orthogonal_map(A, B)


def item_similarity_tables(embeddings, adaptations):
    """save_item_similarity_model (Finetune/pairwise.jl:141-161): embeddings {m: [V_m][E]} (the final eval-mode exports), adaptations
    {m: {"training": (source_ids, target_ids), "test": (...)}} (0-based).  Returns (tables, metrics): tables {"embeddings.{m}": E x V_m
    f32 (Julia's layout), "crossproject.{m}": E x E f32} as serve.load_retrieval_tables reads them, metrics {"{m}.project.training",
    "{m}.project.test"} (avg_norm of the residual)."""
    d = {f"embeddings.{m}": np.ascontiguousarray(np.asarray(embeddings[m], np.float32).T) for m in (0, 1)}
    metrics = {}
    for m in (0, 1):
        A = np.asarray(embeddings[m], np.float64)
        B = np.asarray(embeddings[1 - m], np.float64)
        s, t = adaptations[m]["training"]
        M = cross_medium_map(A, B, s, t)
        metrics[f"{m}.project.training"] = avg_norm(M @ A[np.asarray(s)].T - B[np.asarray(t)].T)
        s2, t2 = adaptations[m]["test"]
        metrics[f"{m}.project.test"] = avg_norm(M @ A[np.asarray(s2)].T - B[np.asarray(t2)].T) if len(s2) else float("nan")
        d[f"crossproject.{m}"] = M.astype(np.float32)
    return d, metrics


# ---- pairwise_metrics.jl: the catalogue metrics the model is accepted by, from the device's ranks
METRIC_KS = (8, 128, 1024)


def dcg_at_k(relevances, k):
    """pairwise_metrics.jl:60-70"""
    score = 0.0
    for i in range(min(k, len(relevances))):
        score += float(relevances[i]) / math.log2(i + 2)
    return score


def _metric_groups(df, ranks):
    """per source in order of first appearance: (weight of its first row, {target: (relevance, rank)} with the LAST row of a repeated
    target, the sum of the relevance column over all of its rows)"""
    groups = {}
    for s, t, r, w, rk in zip(df["source"], df["target"], df["relevance"], df["weight"], ranks):
        g = groups.get(int(s))
        if g is None:
            g = groups[int(s)] = [float(w), {}, []]
        g[1][int(t)] = (float(r), int(rk))
        g[2].append(float(r))
    return groups


def ndcg_at_k(df, ranks, k):
    """ndcg_at_k (pairwise_metrics.jl:72-97) with the sort replaced by its result: ranks[i] = the 1-based position of df's row i's target
    among its source's candidates (LTRModel.pair_ranks; 0: not a candidate).  df: columns source, target, relevance, weight."""
    num = den = 0.0
    for weight, rel, _ in _metric_groups(df, ranks).values():
        dcg = 0.0
        for r, rk in sorted(rel.values(), key=lambda x: x[1]):
            if 1 <= rk <= k:
                dcg += r / math.log2(rk + 1)
        idcg = dcg_at_k(sorted((r for r, _ in rel.values()), reverse=True), k)
        num += (dcg / idcg if idcg > 0 else 0.0) * weight
        den += weight
    return num / den


def recall_at_k(df, ranks, k):
    """recall_at_k (pairwise_metrics.jl:99-123): the relevance found in the top k over the relevance column's sum (repeated rows included)"""
    num = den = 0.0
    for weight, rel, column in _metric_groups(df, ranks).values():
        found = 0.0
        for r, rk in sorted(rel.values(), key=lambda x: x[1]):
            if 1 <= rk <= k:
                found += r
        total = 0.0
        for r in column:
            total += r
        num += found / total * weight
        den += weight
    return num / den


def _natural_sort_key(s):
    import re
    return [int(m.group(2)) if m.group(1) is None else m.group(1) for m in re.finditer(r"([^\d]+)|(\d+)", s)]


def make_metric_dataframe(d):
    """make_metric_dataframe (pairwise_metrics.jl:125-155) without a data-frame library: {"{medium}.{metric}": value} -> (columns, rows),
    `medium` first and the other columns in natural sort order, one row per medium in ascending order"""
    result = {}
    for key, v in d.items():
        task, metric = key.split(".", 1)
        result.setdefault(int(task), {})[metric] = v
    cols = sorted({c for v in result.values() for c in v}, key=_natural_sort_key)
    return ["medium"] + cols, [[m] + [result[m].get(c) for c in cols] for m in sorted(result)]


def metric_frame(pairs, testmask, medium):
    """the data frame of save_metrics (pairwise_metrics.jl:164-172), 0-based ids: rows with cliptype == "medium{m}", score != 0 and
    testmask[source, target] != 0; weight = sqrt(source_popularity)"""
    clip = np.asarray([str(c) for c in pairs["cliptype"]])
    src = np.asarray(pairs["source_matchedid"], np.int64)
    tgt = np.asarray(pairs["target_matchedid"], np.int64)
    score = np.asarray(pairs["score"], np.float64)
    keep = (clip == f"medium{medium}") & (score != 0)
    keep[keep] = np.asarray(testmask)[src[keep], tgt[keep]] != 0
    return {"source": src[keep], "target": tgt[keep], "relevance": score[keep],
            "weight": np.sqrt(np.asarray(pairs["source_popularity"], np.float64)[keep])}


def frame_ranks(model, df):
    """the rank of every row of a metric frame (LTRModel.pair_ranks over its sources in order of first appearance)"""
    rows = {}
    for i, s in enumerate(df["source"]):
        rows.setdefault(int(s), []).append(i)
    ranks = np.zeros(len(df["source"]), np.int32)
    if rows:
        out = model.pair_ranks(list(rows), [df["target"][idx] for idx in rows.values()])
        for idx, r in zip(rows.values(), out):
            ranks[idx] = r
    return ranks


def save_metrics(models_or_exports, pairs, testmasks, datadir, device=0):
    """save_metrics (pairwise_metrics.jl:157-184).  models_or_exports[m]: an LTRModel (its eval-mode export is taken, and held) or the
    export [V_m][E] itself; pairs[m]: the columns of pairs.{m}.csv; testmasks[m]: bool [V_m][V_m].  Writes pairwise.embeddings.csv and
    pairwise.embeddings.npz ("embeddings.{m}": E x V_m, Julia's layout) into datadir; returns (tables, metrics) with metrics =
    {"{m}.nDCG@{k}", "{m}.Recall@{k}"} for k in (8, 128, 1024)."""
    tables, ret = {}, {}
    for medium in sorted(models_or_exports):
        entry = models_or_exports[medium]
        own = not isinstance(entry, LTRModel)
        if own:
            emb = np.ascontiguousarray(entry, np.float32)
            cfg = training_config({medium: emb.shape[0]}, embed_dim=emb.shape[1], batch_size=1, items_per_query=1)
            model = LTRModel(cfg, medium, np.zeros((emb.shape[0], 64), np.float32), dtype="fp32", dropout=0.0, device=device)
            model.set_export(emb)
        else:
            model = entry
            emb = model.embed_all(train_mode=False)
        try:
            model.set_testmask(testmasks[medium])
            df = metric_frame(pairs[medium], testmasks[medium], medium)
            ranks = frame_ranks(model, df)
        finally:
            if own:
                model.close()
        for k in METRIC_KS:
            ret[f"{medium}.nDCG@{k}"] = ndcg_at_k(df, ranks, k)
            ret[f"{medium}.Recall@{k}"] = recall_at_k(df, ranks, k)
        tables[f"embeddings.{medium}"] = np.ascontiguousarray(emb.T)
    np.savez(os.path.join(datadir, "pairwise.embeddings.npz"), **tables)
    cols, rows = make_metric_dataframe(ret)
    with open(os.path.join(datadir, "pairwise.embeddings.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(cols)
        w.writerows(rows)
    return tables, ret
