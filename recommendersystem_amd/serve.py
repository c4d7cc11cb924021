"""Host side of the inference forward: the request -> batch -> model -> response steps of the
reference's embedding server (notebooks/Finetune/embed.py:27-161), on top of `RecommenderModel.inference_forward`
(rsys_infer: fused item table, per-row `rope_input_pos`, per-candidate `token_mask_ids`).

A user's history is a list of events {"medium", "matchedid", "history_max_ts", "status", "rating", "progress",
"history_status", "history_rating"}; `tokenize` merges consecutive events on the same item (the item keeps the first
event's identity and the last event's state, embed.py:39-60), `project` drops events that did not change status or rating
(embed.py:63-71).  Retrieval appends one query token (item -1) and returns the trunk output at that item token; ranking
appends one token per candidate item, each with its own `token_mask_ids` value (candidates see the history but not each
other), and returns the rating head at the candidates' action tokens.
"""
import contextlib

import numpy as np


_STATE_KEYS = ("status", "rating", "progress")
_INT_COLS = ("userid", "rope_input_pos", "token_mask_ids", "gender", "source", "matchedid", "status")


def make_item(ts, medium=0, itemid=-1):
    """A query / candidate token: item `itemid` of `medium` at time `ts` with the masked action state (embed.py:27-36)."""
    return dict(medium=medium, history_max_ts=ts, matchedid=itemid, status=-1, rating=0, progress=0)


def tokenize(user_items):
    """Runs of consecutive events on the same (medium, item) collapse into one token that keeps the first event's fields
    and takes status / rating / progress from the last one (embed.py:39-60)."""
    from itertools import groupby
    tokens = []
    for _, run in groupby(user_items, key=lambda e: (e["medium"], e["matchedid"])):
        run = list(run)
        tok = dict(run[0])
        tok.update({k: run[-1][k] for k in _STATE_KEYS})
        tokens.append(tok)
    return tokens


def project(user_items):
    """Keeps the tokens whose status or rating differs from the item's previous state (embed.py:63-71)."""
    changed = lambda e: e["history_status"] != e["status"] or e["history_rating"] != e["rating"]
    return [e for e in user_items if changed(e)]


def _history(user, max_user_len):
    """projected tokens of a user, newest `max_user_len - 1` kept (one slot is reserved for the query, embed.py:103-106)."""
    hist = project(tokenize(user["items"]))
    return hist[-(max_user_len - 1):] if len(hist) > max_user_len - 1 else hist


def build_batch(users, task, medium, num_items_0, max_user_len=1024, max_ranking_items=1024):
    """The ten (len(users), max_seq_len) arrays of one inference request (embed.py:74-138): history tokens first, then the
    query token (retrieval) or one token per candidate (ranking).  History tokens get positions 0..n-1 and mask id 0; every
    appended token sits at position n, and ranking candidates carry their own index as `token_mask_ids`, which hides them
    from each other (model.py:479-487)."""
    if task not in ("retrieval", "ranking"):
        raise AssertionError(task)
    width = max_user_len + (max_ranking_items if task == "ranking" else 0)
    n = len(users)
    d = {k: np.zeros((n, width), np.int32) for k in _INT_COLS}
    d["time"] = np.zeros((n, width), np.float64)
    d["rating"] = np.zeros((n, width), np.float32)
    d["progress"] = np.zeros((n, width), np.float32)
    for row, u in enumerate(users):
        hist = _history(u, max_user_len)
        if task == "ranking":
            tail = [make_item(u["timestamp"], medium, cand) for cand in u["ranking_items"]]
        else:
            tail = [make_item(u["timestamp"])]
        seq = hist + tail
        L, nh = len(seq), len(hist)
        who = u["user"]
        d["userid"][row, :L] = row + 1
        d["gender"][row, :L] = 0 if who["gender"] is None else who["gender"] + 1
        d["source"][row, :L] = who["source"]
        d["time"][row, :L] = [e["history_max_ts"] for e in seq]
        d["rope_input_pos"][row, :L] = np.minimum(np.arange(L), nh)
        if task == "ranking":
            d["token_mask_ids"][row, nh:L] = np.arange(nh, L)
        d["matchedid"][row, :L] = [e["matchedid"] + (num_items_0 if e["medium"] == 1 else 0) for e in seq]
        d["status"][row, :L] = [e["status"] for e in seq]
        d["rating"][row, :L] = [e["rating"] for e in seq]
        d["progress"][row, :L] = [e["progress"] for e in seq]
    return d


def extract(embs, users, task, medium, max_user_len=1024):
    """Per user, the rows of the model output that answer the request (embed.py:147-161): token 2n is the query's item token
    (retrieval: its trunk output), tokens 2(n+j)+1 are the candidates' action tokens (ranking: their rating-head value)."""
    key = f"{medium}.{task}"
    embs = np.asarray(embs)
    out = []
    for row, u in enumerate(users):
        n = len(_history(u, max_user_len))
        if task == "retrieval":
            out.append({key: embs[row, 2 * n, :].tolist()})
        else:
            rows = 2 * (n + np.arange(len(u["ranking_items"]))) + 1
            out.append({key: embs[row, rows, 0].tolist()})
    return out


def _request_lengths(model, task, max_user_len, max_ranking_items):
    """(max_user_len, max_ranking_items) of a request: the model's `max_sequence_length` is all history + query for retrieval and is
    split between history and candidates for ranking"""
    S = model.config["max_sequence_length"]
    if task == "retrieval":
        max_user_len = S if max_user_len is None else max_user_len
        max_ranking_items = 0
        assert max_user_len == S
    else:
        max_user_len = S // 2 if max_user_len is None else max_user_len
        max_ranking_items = S - max_user_len if max_ranking_items is None else max_ranking_items
        assert max_user_len + max_ranking_items == S
    return max_user_len, max_ranking_items


def _selected_tokens(users, task, S, max_user_len):
    """flat token indices `extract` would read (one per user for retrieval, the candidates' action tokens for ranking) and their
    number per user"""
    index, counts = [], []
    for row, u in enumerate(users):
        n = len(_history(u, max_user_len))
        toks = [2 * n] if task == "retrieval" else list(2 * (n + np.arange(len(u["ranking_items"]))) + 1)
        index += [row * 2 * S + int(t) for t in toks]; counts.append(len(toks))
    return index, counts


def trim_length(live, S):
    """The row length a forward whose longest row has `live` live columns runs at under `trim=True`: whole 64-token attention tiles
    (32 interactions), clamped to the model's S."""
    return min(int(S), 32 * max(1, -(-int(live) // 32)))


def live_columns(d):
    """columns of the longest live prefix of the rows `build_batch` / `_fill_row` filled (live events carry userid != 0, the rest is padding)"""
    uid = np.asarray(d["userid"])
    uid = uid.reshape(-1, uid.shape[-1])
    cols = np.flatnonzero((uid != 0).any(axis=0))
    return int(cols[-1]) + 1 if cols.size else 0


def _row_len(d, S, trim):
    return trim_length(live_columns(d), S) if trim else None


def pack_plan(n_live, S, max_rows):
    """Several users per serving row, as data: user i has `n_live[i]` >= 1 live columns (history + query, or history +
    candidates) and takes ceil(n_live / 32) attention tiles of 32 interactions.  First-fit decreasing over the users (ties in user
    order) into rows where first_column + n_live <= S; a segment starts on a tile boundary and lies inside one row.  Rows keep the
    order they were opened in and a forward is a group of `max_rows` of them.  Returns [(row_len, [(user, row, first_column)])] with
    row = the row inside its forward, segments in (row, column) order and row_len = `trim_length` of the forward's fullest row."""
    n_live = [int(n) for n in n_live]
    if any(n < 1 or n > S for n in n_live):
        raise ValueError(f"pack_plan: every user needs 1 <= live columns <= {S}")
    rows = []                                   # [columns taken (whole tiles), live end, [(user, first_column)]]
    for u in sorted(range(len(n_live)), key=lambda i: -n_live[i]):      # (sorted is stable: ties stay in user order)
        n = n_live[u]
        row = next((r for r in rows if r[0] + n <= S), None)
        if row is None:
            row = [0, 0, []]; rows.append(row)
        row[2].append((u, row[0]))
        row[1] = row[0] + n
        row[0] += 32 * -(-n // 32)
    plan = []
    for r0 in range(0, len(rows), max_rows):
        group = rows[r0:r0 + max_rows]
        plan.append((trim_length(max(r[1] for r in group), S), [(u, k, c0) for k, r in enumerate(group) for u, c0 in r[2]]))
    return plan


def build_packed(users, media, task, plan_forward, num_items_0, max_user_len=1024, max_ranking_items=1024, adapter_slots=None, hists=None):
    """One forward of `pack_plan` as arrays.  `users` / `media`: the request's users and each one's medium (one int: the same for all);
    `plan_forward` = (row_len, [(user, row, first_column)]).  A user's segment is the live prefix of its own `build_batch` row --
    `rope_input_pos` and the candidates' `token_mask_ids` stay relative to the segment -- except `userid`: 1 + the segment's place in
    the forward, distinct within a row; the columns between segments are zero.  Returns (d, index, tiles): the ten (rows, S) arrays,
    per segment the flat token indices row * 2S + token `extract` would read, and the (rows, ceil(S / 32)) int32 map of
    `adapter_slots["{medium}.{task}"]` over each segment's tiles, -1 elsewhere (None without `adapter_slots`).  `hists`: the users'
    `_history(user, max_user_len)` when the caller has them already (each history is tokenised once per request)."""
    width = max_user_len + (max_ranking_items if task == "ranking" else 0)
    _, placed = plan_forward
    rows = 1 + max(r for _, r, _ in placed)
    d = _empty_rows(rows, width)
    tiles = np.full((rows, -(-width // 32)), -1, np.int32) if adapter_slots else None
    index = []
    for k, (u, row, c0) in enumerate(placed):
        medium = int(media if np.ndim(media) == 0 else media[u])
        user = users[u]
        hist = _history(user, max_user_len) if hists is None else hists[u]
        ranking = task == "ranking"
        seq = hist + ([make_item(user["timestamp"], medium, c) for c in user["ranking_items"]] if ranking else [make_item(user["timestamp"])])
        n, nh = len(seq), len(hist)
        if c0 % 32 or c0 + n > width or (ranking and n - nh > max_ranking_items) or d["userid"][row, c0:c0 + n].any():
            raise ValueError(f"build_packed: user {u} does not fit at column {c0} of row {row}")
        _fill_row(d, row, seq, nh, user["user"], num_items_0, ranking, c0)         # (the row `build_batch` fills for this user alone)
        d["userid"][row, c0:c0 + n] = k + 1
        toks = [2 * nh] if not ranking else [2 * (nh + j) + 1 for j in range(n - nh)]      # (`_selected_tokens` of the user's own row)
        index.append([row * 2 * width + 2 * c0 + t for t in toks])
        if tiles is not None:
            tiles[row, c0 // 32:-(-(c0 + n) // 32)] = adapter_slots[f"{medium}.{task}"]
    return d, index, tiles


def _predict_packed(model, requests, task, max_user_len, max_ranking_items):
    """`predict` / `predict_mixed` with several users per row: the forwards of `pack_plan` over the users that have a token to read,
    each at its own trimmed length with one adapter slot per tile; results in request order."""
    S = model.config["max_sequence_length"]
    max_user_len, max_ranking_items = _request_lengths(model, task, max_user_len, max_ranking_items)
    n0 = model.config["vocab_sizes"]["0_matchedid"]
    users = [u for u, _ in requests]
    media = [int(m) for _, m in requests]
    out = [{f"{m}.{task}": []} for m in media]
    tail = [1 if task == "retrieval" else len(u["ranking_items"]) for u in users]
    live = [i for i, t in enumerate(tail) if t]
    hists = [_history(u, max_user_len) for u in users]               # once per user
    n_live = [len(hists[i]) + tail[i] for i in live]
    slots = getattr(model, "adapter_slots", None)
    for forward in pack_plan(n_live, S, model.max_rows):
        sub = (forward[0], [(live[u], r, c0) for u, r, c0 in forward[1]])
        d, index, tiles = build_packed(users, media, task, sub, n0, max_user_len, max_ranking_items, slots or None, hists)
        kw = dict(tile_adapters=tiles) if tiles is not None else {}
        vals = model.inference_select(d, task, [t for ix in index for t in ix], row_len=forward[0], **kw)
        at = 0
        for (u, _, _), ix in zip(sub[1], index):
            out[u] = {f"{media[u]}.{task}": (vals[at].tolist() if task == "retrieval" else vals[at:at + len(ix)].tolist())}
            at += len(ix)
    return out


def compact_top_rows(n_sel, n_tokens, cap):
    """First count rule of the serving compact top (restates csrc/model_forward.hip serving_top_mode, as `_plan_segments`
    restates the library's packing): a forward of `n_tokens` tokens that reports `n_sel` of them runs the last layer's tail and the
    final norm on those rows only iff the selection fits the compact buffers (`cap` rows) and is at most half of the tokens."""
    return 1 <= n_sel <= cap and 2 * n_sel <= n_tokens


def compact_top_selected_attention(n_sel, rows, row_len):
    """Second count rule: the last layer's attention runs for the selected queries only (attn_sel_kernel) iff there is at most one of
    them per 64-token tile on average, `n_sel <= rows * ceil(2 row_len / 64)` -- it then reads no more K | V bytes than the tile kernel
    would.  A count rule, not a measured threshold."""
    return n_sel <= rows * -(-2 * row_len // 64)


def compact_top_mode(n_sel, rows, row_len, cap, kind="select"):
    """What the library reports as "infer.top" for an inference pass under rsys_serving_compact_top_set on a model that has the compact
    buffers: kind "store" (a K/V-cache store pass) -> 3; "select" / "candidates" (a pass that reports `n_sel` tokens of `rows` rows of
    2 `row_len` tokens) -> 0 dense, 1 compact tail behind the dense attention, 2 compact tail behind the selected-query attention
    (never for candidate rows, whose keys live in the cache); n_sel = None (rsys_infer without a selection) -> 0."""
    if kind == "store":
        return 3
    if n_sel is None or not compact_top_rows(n_sel, rows * 2 * row_len, cap):
        return 0
    return 2 if kind == "select" and compact_top_selected_attention(n_sel, rows, row_len) else 1


@contextlib.contextmanager
def _compact_top(model):
    """rsys_serving_compact_top_set for the length of a call, restored on every exit path"""
    before = model.serving_compact_top()
    model.serving_compact_top(True)
    try:
        yield
    finally:
        model.serving_compact_top(before)


def predict(model, users, task, medium, max_user_len=None, max_ranking_items=None, trim=False, pack=False, compact_top=False):
    """embed.py:74-161 on the HIP model (`model.config["forward"]` semantics = inference): sequence length of the request =
    the model's `max_sequence_length` (retrieval: all of it is history + query; ranking: split between history and candidates).
    A model built by `get_models` (it has an `adapter_slots` map) runs every row with the adapter of "{medium}.{task}".
    `trim=True`: the forward runs at `trim_length` of the batch's longest live row instead of S (the padding behind it is dropped, which
    is exact: no live token attends it).
    `pack=True` (implies trimming): several users share a row, each in a segment of whole 64-token attention tiles (`pack_plan`), and any
    number of users is served in forwards of at most `max_rows` rows; results are in the users' order.
    `compact_top=True` (rsys_serving_compact_top_set for the length of the call): the last layer runs only where its outputs are read
    (`compact_top_mode`); values agree with the dense pass to rounding."""
    if compact_top:
        with _compact_top(model):
            return predict(model, users, task, medium, max_user_len, max_ranking_items, trim, pack)
    if pack:
        return _predict_packed(model, [(u, medium) for u in users], task, max_user_len, max_ranking_items)
    S = model.config["max_sequence_length"]
    max_user_len, max_ranking_items = _request_lengths(model, task, max_user_len, max_ranking_items)
    d = build_batch(users, task, medium, model.config["vocab_sizes"]["0_matchedid"], max_user_len, max_ranking_items)
    if not hasattr(model, "inference_select"):           # (a model that only has the reference's call: the full tensor, then extract)
        return extract(model.inference_forward(d, task), users, task, medium, max_user_len)
    # only the tokens `extract` would read leave the device (one row per user for retrieval, the candidates' action tokens for
    # ranking) instead of the (rows, 2S, D) tensor
    index, counts = _selected_tokens(users, task, S, max_user_len)
    key = f"{medium}.{task}"
    if not index:
        return [{key: []} for _ in users]
    slots = getattr(model, "adapter_slots", None)
    kw = dict(row_len=_row_len(d, S, trim)) if trim else {}
    if slots:
        vals = model.inference_select(d, task, index, adapters=[slots[key]] * len(users), **kw)
    else:
        vals = model.inference_select(d, task, index, **kw)
    out, at = [], 0
    for c in counts:
        out.append({key: (vals[at].tolist() if task == "retrieval" else vals[at:at + c].tolist())}); at += c
    return out


def rank_cache_plan(n_hist, n_cand, S, max_rows):
    """The calls `predict_ranking_full` makes for users with `n_hist[i]` >= 1 history events and `n_cand[i]` candidates, as data: a list of
    waves of at most `max_rows` users; a wave is (store, batches) with store = [(user, slot, n_hist)] (slot = the user's place in the
    wave, one history row each) and batches = lists of at most `max_rows` candidate rows (user, slot, first candidate, candidates <= S,
    rope_input_pos = n_hist), users in order and a user's rows in candidate order -- so the concatenated outputs of a wave's batches are
    the users' values in order."""
    waves = []
    for u0 in range(0, len(n_hist), max_rows):
        users = range(u0, min(u0 + max_rows, len(n_hist)))
        store = [(u, u - u0, int(n_hist[u])) for u in users]
        rows = [(u, u - u0, c0, min(S, int(n_cand[u]) - c0), int(n_hist[u])) for u in users for c0 in range(0, int(n_cand[u]), S)]
        waves.append((store, [rows[r0:r0 + max_rows] for r0 in range(0, len(rows), max_rows)]))
    return waves


def _plan_segments(lengths, S, max_rows):
    """One stage of `rank_cache_pack_plan`: segments of `lengths[i]` >= 1 columns into forwards [(row_len, [(segment, row, first_column)])].
    The packed layout is `pack_plan`'s (first-fit decreasing, ties in order, rows in the order they were opened, forwards of `max_rows`
    rows at `trim_length` of their fullest row); it is taken only if it needs fewer forwards than one segment per row at its trim
    length, or as many forwards and fewer tokens.  Otherwise every segment gets a row of its own, at column 0, in segment order."""
    packed = pack_plan(lengths, S, max_rows)
    single = [(trim_length(max(lengths[r0:r0 + max_rows]), S), [(r0 + k, k, 0) for k in range(len(lengths[r0:r0 + max_rows]))])
              for r0 in range(0, len(lengths), max_rows)]
    tokens = lambda plan: sum(row_len * (1 + max(r for _, r, _ in placed)) for row_len, placed in plan)
    if len(packed) < len(single) or (len(packed) == len(single) and tokens(packed) < tokens(single)):
        return packed
    return single


def rank_cache_pack_plan(n_hist, n_cand, S, max_rows, slots):
    """`rank_cache_plan` with several users per row, as data, for users with `n_hist[i]` in [1, S] history events and
    `n_cand[i]` >= 0 candidates.  Waves hold at most `slots` users, in user order; slot = the user's place in its wave.  A wave is
    (stores, candidates): `stores` = forwards (row_len, [(user, row, first_column, n_hist, slot)]) over the wave's histories, `candidates`
    = forwards (row_len, [(user, row, first_column, first_candidate, n_cand <= S, slot)]) over its candidate lists cut into chunks of at
    most S.  Segments start on a multiple of 32 columns, lie inside one row and share no 32-column tile; each stage is planned by
    `_plan_segments`, so where packing saves neither a forward nor tokens the stage is one segment per row at column 0."""
    n_hist = [int(n) for n in n_hist]; n_cand = [int(n) for n in n_cand]
    if len(n_hist) != len(n_cand) or any(n < 1 or n > S for n in n_hist) or any(n < 0 for n in n_cand) or slots < 1 or max_rows < 1:
        raise ValueError(f"rank_cache_pack_plan: 1 <= n_hist <= {S} and n_cand >= 0 per user, slots >= 1, max_rows >= 1")
    waves = []
    for u0 in range(0, len(n_hist), slots):
        users = list(range(u0, min(u0 + slots, len(n_hist))))
        stores = [(row_len, [(users[k], row, c0, n_hist[users[k]], k) for k, row, c0 in placed])
                  for row_len, placed in _plan_segments([n_hist[u] for u in users], S, max_rows)]
        chunks = [(u, u - u0, c, min(S, n_cand[u] - c)) for u in users for c in range(0, n_cand[u], S)]
        cands = [(row_len, [(chunks[k][0], row, c0, chunks[k][2], chunks[k][3], chunks[k][1]) for k, row, c0 in placed])
                 for row_len, placed in (_plan_segments([c[3] for c in chunks], S, max_rows) if chunks else [])]
        waves.append((stores, cands))
    return waves


def _predict_ranking_packed(model, users, medium, full, hists, out, cache_slots):
    """`predict_ranking_full`'s cached part over the plan of `rank_cache_pack_plan`: every forward at its own trimmed length"""
    S = model.config["max_sequence_length"]
    n0 = model.config["vocab_sizes"]["0_matchedid"]
    key = f"{medium}.ranking"
    slots = getattr(model, "adapter_slots", None)
    adapter = slots[key] if slots else None
    n_slots = min(sum(1 for h in hists if h), int(cache_slots) if cache_slots else 4 * model.max_rows)
    if getattr(model, "rank_cache_slots", 0) < n_slots:
        model.rank_cache_reserve(n_slots)
    plan = rank_cache_pack_plan([len(hists[i]) for i in full], [len(users[i]["ranking_items"]) for i in full], S, model.max_rows, n_slots)
    vals = {i: np.zeros(len(users[i]["ranking_items"]), np.float32) for i in full}
    for stores, cands in plan:
        for row_len, placed in stores:
            d = _empty_rows(1 + max(p[1] for p in placed), S)
            for k, (u, row, c0, nh, _) in enumerate(placed):
                _fill_row(d, row, hists[full[u]], nh, users[full[u]]["user"], n0, False, c0)
                d["userid"][row, c0:c0 + nh] = k + 1           # (distinct among the segments of the forward: no history sees another)
            model.rank_cache_store_packed(d, [(row, c0, nh, slot) for _, row, c0, nh, slot in placed], adapters=adapter, row_len=row_len)
        for row_len, placed in cands:
            d = _empty_rows(1 + max(p[1] for p in placed), S)
            for u, row, c0, first, n, _ in placed:
                who = users[full[u]]
                seq = [make_item(who["timestamp"], medium, c) for c in who["ranking_items"][first:first + n]]
                _fill_row(d, row, seq, 0, who["user"], n0, False, c0)
                d["rope_input_pos"][row, c0:c0 + n] = len(hists[full[u]])     # (as the candidate rows of the unpacked path; the call sets the positions itself)
            v = model.rank_cache_candidates_packed(d, [(row, c0, n, slot) for _, row, c0, _, n, slot in placed], adapters=adapter, row_len=row_len)
            at = 0
            for u, _, _, first, n, _ in placed:
                vals[full[u]][first:first + n] = v[at:at + n]; at += n
    for i in full:
        out[i] = {key: vals[i].tolist()}
    return out


def predict_ranking_full(model, users, medium, trim=False, pack=False, cache_slots=None, compact_top=False):
    """`predict(model, users, "ranking", medium)` on the reference's row (embed.py:74-161 with max_user_len = S): every user is ranked
    on its newest S - 1 history events, whatever the number of candidates, instead of the newest S // 2 - 1 that share a row with the
    candidates.  Each history is tokenised and projected once and runs once (one `rank_cache_store` per wave of `max_rows` users);
    the candidates run against the cached K / V in rows of up to S (a user's candidates may span rows, several users' rows share a
    forward).  Users with an empty history go through `predict`, one row per chunk of S - S // 2 candidates as `render` cuts them, so
    their values are what `render` gives today.  Returns what `predict` returns, for any number of candidates.  `trim=True`: every
    store and candidate forward runs at `trim_length` of its longest row; slots, waves and chunks are unchanged.
    `pack=True` (implies trimming): the users with a history run by `rank_cache_pack_plan` -- several histories per store row, several
    users' candidate chunks per candidate row, waves of up to `cache_slots` (default 4 x max_rows) users; min(users with a history,
    that many) cache slots are reserved when the model holds fewer -- which, as every `rank_cache_reserve` of a new size, drops what
    a caller had stored.  Users with an empty history and users without candidates go the ways they go without it.
    `compact_top=True` (rsys_serving_compact_top_set for the length of the call): every store forward ends at its last K | V copy (the
    slots hold the same bits) and the candidate forwards run the last layer's tail on the candidates' action tokens only."""
    if compact_top:
        with _compact_top(model):
            return predict_ranking_full(model, users, medium, trim, pack, cache_slots)
    S = model.config["max_sequence_length"]
    n0 = model.config["vocab_sizes"]["0_matchedid"]
    key = f"{medium}.ranking"
    out = [None] * len(users)
    hists = [_history(u, S) for u in users]
    chunk = S - S // 2
    for i in (i for i, h in enumerate(hists) if not h):
        # as `render` runs them: one `predict` row per chunk of S - S // 2 candidates, so the values are the ones that path gives
        # (with an empty history they depend on where the chunks are cut: candidate 0 of a row carries mask id 0)
        items, vals = users[i]["ranking_items"], []
        for c0 in range(0, len(items), chunk):
            vals += predict(model, [dict(users[i], ranking_items=items[c0:c0 + chunk])], "ranking", medium, trim=trim)[0][key]
        out[i] = {key: vals}
    full = [i for i, h in enumerate(hists) if h]
    for i in full:
        if not users[i]["ranking_items"]:
            out[i] = {key: []}
    full = [i for i in full if users[i]["ranking_items"]]
    if not full:
        return out
    if pack:
        return _predict_ranking_packed(model, users, medium, full, hists, out, cache_slots)
    slots = getattr(model, "adapter_slots", None)
    adapter = slots[key] if slots else None
    max_rows = model.max_rows
    if getattr(model, "rank_cache_slots", 0) < min(max_rows, len(full)):
        model.rank_cache_reserve(max_rows)
    plan = rank_cache_plan([len(hists[i]) for i in full], [len(users[i]["ranking_items"]) for i in full], S, max_rows)
    for store, batches in plan:
        d = _empty_rows(len(store), S)
        for row, (k, _, nh) in enumerate(store):
            _fill_row(d, row, hists[full[k]], nh, users[full[k]]["user"], n0, False)
        kw = dict(row_len=_row_len(d, S, True)) if trim else {}
        model.rank_cache_store(d, [s[2] for s in store], [s[1] for s in store], adapters=adapter, **kw)
        vals = {k: [] for k, _, _ in store}
        for rows in batches:
            d = _empty_rows(len(rows), S)
            for row, (k, _, c0, n, nh) in enumerate(rows):
                u = users[full[k]]
                seq = [make_item(u["timestamp"], medium, c) for c in u["ranking_items"][c0:c0 + n]]
                _fill_row(d, row, seq, 0, u["user"], n0, False)
                d["rope_input_pos"][row, :] = nh     # (the reference's value for every candidate; the call sets the positions itself from the
                                                     #  slot, so this only keeps the uploaded row equal to the reference's candidate events)
            kw = dict(row_len=_row_len(d, S, True)) if trim else {}
            v = model.rank_cache_candidates(d, [r[1] for r in rows], [r[3] for r in rows], adapters=adapter, **kw)
            at = 0
            for k, _, _, n, _ in rows:
                vals[k] += v[at:at + n].tolist(); at += n
        for k, _, _ in store:
            out[full[k]] = {key: vals[k]}
    return out


def predict_mixed(model, requests, task, max_user_len=None, max_ranking_items=None, trim=False, pack=False, compact_top=False):
    """`predict` for users of both media in ONE forward: `requests` = [(user, medium), ...]; row i of the batch is the row
    `build_batch([user_i], task, medium_i, ...)` builds and runs with the adapter slot `model.adapter_slots[f"{medium_i}.{task}"]`
    (embed.jl:5-84 keeps one queue per (medium, task) on one GPU; single-user inference is launch-bound, so sharing a forward
    is what the shared trunk buys).  Result i is keyed "{medium_i}.{task}" like `predict`'s.  `pack=True`: users of both media share
    rows as well (`pack_plan`, one adapter slot per tile).  `compact_top=True`: as `predict`'s."""
    if compact_top:
        with _compact_top(model):
            return predict_mixed(model, requests, task, max_user_len, max_ranking_items, trim, pack)
    slots = getattr(model, "adapter_slots", None)
    if not slots:
        raise ValueError("predict_mixed: the model has no adapter_slots map (build it with get_models)")
    if not requests:
        return []
    if pack:
        return _predict_packed(model, requests, task, max_user_len, max_ranking_items)
    S = model.config["max_sequence_length"]
    max_user_len, max_ranking_items = _request_lengths(model, task, max_user_len, max_ranking_items)
    n0 = model.config["vocab_sizes"]["0_matchedid"]
    parts = [build_batch([u], task, int(m), n0, max_user_len, max_ranking_items) for u, m in requests]
    d = {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0]}    # (every row keeps userid 1: attention never crosses batch rows)
    users = [u for u, _ in requests]
    index, counts = _selected_tokens(users, task, S, max_user_len)
    keys = [f"{int(m)}.{task}" for _, m in requests]
    if not index:
        return [{k: []} for k in keys]
    kw = dict(row_len=_row_len(d, S, True)) if trim else {}
    vals = model.inference_select(d, task, index, adapters=[slots[k] for k in keys], **kw)
    out, at = [], 0
    for k, c in zip(keys, counts):
        out.append({k: (vals[at].tolist() if task == "retrieval" else vals[at:at + c].tolist())}); at += c
    return out


ADAPTER_TASKS = {"watch": "retrieval", "rating": "ranking"}      # embed.py:182


def get_models(base, loras, config, device=0, dtype="bf16", max_rows=4, model_cls=None):
    """Finetune/embed.py:180-255 (`load_model` + `get_models`) on one base model: the consumer of
    `checkpoint.dedup_finetune_models`.  `base`: the shared trunk (`.npz`-layout dict, keys "model/..."); `loras`: the LoRA-only
    blobs, either {"{medium}.{metric}": blob} (metric watch / rating) or a list in the reference's order (0.watch, 0.rating, 1.watch,
    1.rating, Finetune/run.jl:9-13).  Builds ONE model (finetune off, forward = inference), loads the trunk once, puts every adapter
    into a bank slot and records `model.adapter_slots = {"0.retrieval": s, "0.ranking": s, "1.retrieval": s, "1.ranking": s}`."""
    order = [(m, metric) for m in (0, 1) for metric in ("watch", "rating")]
    if not isinstance(loras, dict):
        loras = list(loras)
        if len(loras) != len(order):
            raise ValueError(f"get_models: {len(loras)} adapters, expected {len(order)} (0.watch, 0.rating, 1.watch, 1.rating)")
        loras = {f"{m}.{metric}": blob for (m, metric), blob in zip(order, loras)}
    strip = lambda blob: {k[len("model/"):]: v for k, v in blob.items() if k.startswith("model/")}
    adapters = {}
    for m, metric in order:
        key = f"{m}.{metric}"
        if key not in loras:
            raise KeyError(f"get_models: no adapter for {key}")
        sd = {k: v for k, v in strip(loras[key]).items() if "lora_" in k}
        if not sd:
            raise KeyError(f"get_models: adapter {key} has no lora keys")
        adapters[key] = sd
    trunk = {k: v for k, v in strip(base).items() if "lora_" not in k}
    if not trunk:
        raise KeyError("get_models: the base has no trunk keys")
    cfg = dict(config)
    cfg["finetune"] = False
    cfg["forward"] = "inference"
    if model_cls is None:
        from .model import RecommenderModel as model_cls
    model = model_cls(cfg, device=device, dtype=dtype, max_rows=max_rows)
    model.load_state_dict(trunk, strict=False)
    model.adapter_slots = {}
    for slot, (m, metric) in enumerate(order):
        model.load_adapter(slot, adapters[f"{m}.{metric}"])
        model.adapter_slots[f"{m}.{ADAPTER_TASKS[metric]}"] = slot
    return model


def register_transformer(model, path):
    """Finetune/register.py:14-36: the serving registry `model.registry.h5` -- the item table split by medium (the
    retrieval scores are softmax(table . user embedding), Finetune/embed.jl:86-90) and the rating offset of each medium."""
    from . import h5
    n0 = model.config["vocab_sizes"]["0_matchedid"]
    embs = model.item_embeddings()
    mean = np.float64(model.config["rating_mean"])
    h5.write_h5(path, {"0.watch.weight": embs[:n0], "1.watch.weight": embs[n0:], "0.rating_mean": mean, "1.rating_mean": mean}, blosc=None)


def compute_retrieval(registry, medium, user, idxs=None):
    """Finetune/embed.jl:86-90: p = softmax(table_m . u) over the medium's items (optionally at `idxs`), times the
    registry's retrieval coefficient when it has one (`{m}.retrieval.coefs`, fitted by Finetune/regress.jl)."""
    logits = np.asarray(registry[f"{medium}.watch.weight"], np.float64) @ np.asarray(user[f"{medium}.retrieval"], np.float64)
    p = np.exp(logits - logits.max())
    p /= p.sum()
    if idxs is not None:
        p = p[np.asarray(idxs)]
    coefs = registry.get(f"{medium}.retrieval.coefs")
    return (p * np.asarray(coefs).reshape(-1)[0] if coefs is not None else p).astype(np.float32)


def compute_ranking(registry, medium, user):
    """Finetune/embed.jl:92-96: blend of the medium's mean rating and the model's rating predictions with the registry's
    coefficients (`{m}.rating.coefs` = [baseline, model]); without coefficients the model's prediction alone."""
    r_masked = np.asarray(user[f"{medium}.ranking"], np.float64)
    coefs = registry.get(f"{medium}.rating.coefs")
    if coefs is None:
        return r_masked.astype(np.float32)
    c = np.asarray(coefs, np.float64).reshape(-1)
    return (c[0] * float(np.asarray(registry[f"{medium}.rating_mean"])) + c[1] * r_masked).astype(np.float32)


# Inference/render.jl:13-23
STATUS_DELETED, STATUS_PLANNED = 3, 5


def watched_exclusions(items, medium):
    """The first two masks of Inference/render.jl:255-266 as medium-local ids (sorted, int32): item 0 (`p[1] = -Inf`, the default
    id of long-tail items) and every item of `medium` whose status -- the last event's, as render.jl's per-user status dict keeps
    it -- is neither deleted (3) nor planned (5).  Relation masks and item similarity stay with the host (exclusions / `prior`)."""
    status = {}
    for e in items:
        if int(e["medium"]) == int(medium):
            status[int(e["matchedid"])] = int(e["status"])
    out = {0} | {i for i, s in status.items() if s not in (STATUS_DELETED, STATUS_PLANNED)}
    return np.array(sorted(out), np.int32)


def retrieve(model, embeds, medium, k, groups=None, exclude=None, prior=None, coefs=None):
    """Retrieval candidates on the device (Inference/render.jl:240-333 without its relation masks, which arrive as `exclude` or a
    -inf `prior`): `embeds` are the "{medium}.retrieval" vectors `predict` returns (dicts) or an (n, D) array; `groups` one group id
    per embedding (a request's users share one, render.jl sums their log-probabilities) or None (one group each); `exclude` a list
    of per-group medium-local id arrays (ragged); `prior` (n_groups, V_m) added to the scores; `coefs` the registry's retrieval
    coefficient (`compute_retrieval`'s factor: adds log(coef) per user, the order does not change).  Returns one (ids, scores)
    pair per group, best first, at most k items (fewer when fewer are admissible)."""
    if medium not in (0, 1):
        raise ValueError("retrieve: medium must be 0 or 1")
    key = f"{medium}.retrieval"
    rows = [e[key] if isinstance(e, dict) else e for e in embeds]
    q = np.asarray(rows, np.float32)
    if q.ndim != 2 or q.shape[0] == 0:
        raise ValueError("retrieve: embeds must be a non-empty list of vectors")
    if q.shape[1] != model.config["embed_dim"]:
        raise ValueError(f"retrieve: embeddings have {q.shape[1]} values, the model {model.config['embed_dim']}")
    Vm = model.config["vocab_sizes"][f"{medium}_matchedid"]
    if not 1 <= int(k) <= min(Vm, 8192):
        raise ValueError(f"retrieve: k must be in [1, {min(Vm, 8192)}]")
    g = np.arange(q.shape[0], dtype=np.int32) if groups is None else np.asarray(groups, np.int64).reshape(-1)
    if g.size != q.shape[0]:
        raise ValueError(f"retrieve: {g.size} group ids for {q.shape[0]} embeddings")
    if g.min() < 0:
        raise ValueError("retrieve: group ids must be >= 0")
    ng = int(g.max()) + 1
    members = np.bincount(g, minlength=ng)
    if (members == 0).any():
        raise ValueError(f"retrieve: groups without an embedding: {np.flatnonzero(members == 0).tolist()}")
    if exclude is not None:
        if len(exclude) != ng:
            raise ValueError(f"retrieve: exclude has {len(exclude)} lists for {ng} groups")
        for e in exclude:
            e = np.asarray(e).reshape(-1)
            if e.size and (e.min() < 0 or e.max() >= Vm):
                raise ValueError(f"retrieve: exclusion ids must be in [0, {Vm})")
    if prior is not None and np.shape(prior) != (ng, Vm):
        raise ValueError(f"retrieve: prior has shape {np.shape(prior)}, expected {(ng, Vm)}")
    ids, scores, counts = model.retrieve_topk(q, medium, int(k), group=None if groups is None else g.astype(np.int32),
                                              prior=prior, exclude=exclude)
    out = []
    for j in range(ng):
        n = int(counts[j])
        s = scores[j, :n]
        if coefs is not None:
            s = (s.astype(np.float64) + members[j] * np.log(float(np.asarray(coefs).reshape(-1)[0]))).astype(np.float32)
        out.append((ids[j, :n].copy(), s))
    return out


# ---------------------------------------------------------------- whole retrieval requests (render.jl `retrieval(state)`)
RELATION_KINDS = ("dependencies", "recaps", "adaptations")


def julia_csc(a):
    """A relation matrix as `RecommenderModel.set_retrieval_relations` takes it: a Julia-shaped SparseMatrixCSC (a dict or object
    with 1-based `colptr` / `rowval`, `nzval` and `m` / `n`, as JLD2 stores it) becomes a 0-based (indptr, indices, data, shape);
    a (indptr, indices, data, shape) tuple or an object with those attributes (scipy CSC) is 0-based already and passes through."""
    get = (lambda k: a[k]) if isinstance(a, dict) else (lambda k: getattr(a, k))
    has = (lambda k: k in a) if isinstance(a, dict) else (lambda k: hasattr(a, k))
    if has("colptr"):
        shape = (int(np.asarray(get("m"))), int(np.asarray(get("n"))))
        return (np.asarray(get("colptr"), np.int64) - 1, np.asarray(get("rowval"), np.int64) - 1, np.asarray(get("nzval"), np.float32),
                shape)
    return a


def load_retrieval_tables(model, relations, item_similarity, released=None):
    """Loads render.jl's serving tables onto the device once (`relations`, `item_similarity`: its own dicts, keyed "{m}.dependencies",
    "{m}.recaps", "{m}.adaptations", "embeddings.{m}", "crossproject.{m}").  Relation matrices are Julia-shaped SparseMatrixCSC dicts
    or 0-based CSC tuples / objects (`julia_csc`); "embeddings.{m}" is Julia's dim x V_m matrix (an array of shape (V_m, dim) is taken
    as its transpose); "crossproject.{m}" the dim x dim matrix as Julia indexes it.  `released`: {m: mask or ids} (render.jl's
    `keys(get_media_info(m))`, 0-based) or None.  A medium whose keys are absent is left as it is."""
    for m in (0, 1):
        if all(f"{m}.{kind}" in relations for kind in RELATION_KINDS):
            model.set_retrieval_relations(m, *(julia_csc(relations[f"{m}.{kind}"]) for kind in RELATION_KINDS))
        if f"embeddings.{m}" in item_similarity:
            e = np.asarray(item_similarity[f"embeddings.{m}"], np.float32)
            Vm = model.config["vocab_sizes"][f"{m}_matchedid"]
            if e.ndim == 2 and e.shape[1] == Vm:
                e = e.T
            model.set_item_similarity(m, e, item_similarity.get(f"crossproject.{m}"))
        if released is not None and m in released:
            model.set_released(m, released[m])


def state_weights(states):
    """The query weights of request states: `state["users"][i]["weight"]` per user in user order and
    `state["items"][i]["weight"]` per selected item in item order, float32, an absent key = 1.0.  Returns (user_weights,
    selected_weights); a kind for which no user / no item of any state carries the key is None -- unweighted, the library's setter is
    then not called for it.  A NaN or infinite weight raises."""
    users = [u for st in states for u in st["users"]]
    items = [a for st in states for a in st.get("items", ())]      # (`ranking` takes states without selected items)
    out = []
    for entries in (users, items):
        if not any("weight" in e for e in entries):
            out.append(None)
            continue
        w = np.asarray([float(e.get("weight", 1.0)) for e in entries], np.float32)
        if not np.isfinite(w).all():
            raise ValueError("query weights must be finite")
        out.append(w)
    return out[0], out[1]


def state_texts(states, medium=None):
    """The text queries of request states: `state["texts"] = [{"embedding": array[Q], "weight": w}, ...]`, optional, in
    state order and text order.  Returns None when no state (of `medium`, if given) holds a text -- the library's setter is then not
    called -- else (embeddings (n, Q) float32, group (n,) int32 = the state's index in `states`, weights (n,) float32 or None).  As in
    `state_weights` an absent "weight" is 1.0, weights is None when no text carries the key, and a NaN or infinite weight or embedding
    value raises."""
    x, group, entries = [], [], []
    for g, st in enumerate(states):
        if medium is not None and int(st["medium"]) != medium:
            continue
        for t in st.get("texts", ()):
            x.append(np.asarray(t["embedding"], np.float32).reshape(-1))
            group.append(g)
            entries.append(t)
    if not x:
        return None
    if len({v.size for v in x}) != 1:
        raise ValueError("text queries: the embeddings of one request must have one width")
    x = np.stack(x)
    if not np.isfinite(x).all():
        raise ValueError("text queries: embeddings must be finite")
    w = None
    if any("weight" in e for e in entries):
        w = np.asarray([float(e.get("weight", 1.0)) for e in entries], np.float32)
        if not np.isfinite(w).all():
            raise ValueError("query weights must be finite")
    return x, np.asarray(group, np.int32), w


def _texts_before(model, states, search, media=None):
    """`RecommenderModel.query_texts_set` for the texts of `states`: one call per medium that has texts, with `search[medium]` (a
    SearchModel on the medium's item table).  `media`: the media to look at (default: those of the states); groups are indices into
    `states`.  Every medium with texts is checked against `search` before the first call, so a missing entry raises with nothing set;
    if a later call fails, the sets of the earlier ones are cleared.  States without a "texts" entry call nothing.  Returns the media set."""
    sets = [(m, state_texts(states, m)) for m in sorted({int(st["medium"]) for st in states} if media is None else media)]
    sets = [(m, t) for m, t in sets if t is not None]
    for m, _ in sets:
        if not search or m not in search:
            raise ValueError(f"a state of medium {m} holds text queries but `search` has no SearchModel for it")
    done = []
    try:
        for m, t in sets:
            model.query_texts_set(search[m], m, *t)
            done.append(m)
    except BaseException:
        _texts_clear(model, done)
        raise
    return done


def _texts_clear(model, media):
    for m in media:
        model.query_texts_set(None, m, np.zeros((0, 1), np.float32), np.zeros(0, np.int32))


@contextlib.contextmanager
def _texts(model, states, search, media=None):
    """the texts of `states` set for the request that runs in the body, immediately before it; if the body raises before the library has
    consumed them (a check of the Python wrapper), they are cleared, so that no later request finds them"""
    done = _texts_before(model, states, search, media)
    try:
        yield
    except BaseException:
        _texts_clear(model, done)
        raise


def _users_and_selected(states, who=None, selected=True):
    """What every request path reads off its states, one group per state: the users' dicts in state and user order, their group ids,
    each user's list items as (medium, matchedid, status) in list order -- every entry, duplicates and all statuses included -- and
    (selected=True) each state's selected items as (medium, matchedid) in order.  `who`: a state without users raises in its name."""
    users, group, hist, sel = [], [], [], []
    for g, st in enumerate(states):
        if who and not st["users"]:
            raise ValueError(f"{who}: every state needs at least one user")
        for u in st["users"]:
            users.append(u)
            group.append(g)
            hist.append([(int(x["medium"]), int(x["matchedid"]), int(x["status"])) for x in u["user"]["items"]])
        if selected:
            sel.append([(int(a["medium"]), int(a["matchedid"])) for a in st["items"]])
    return users, np.asarray(group, np.int32), hist, sel


def _embeds(users, key):
    """the users' `key` embeddings as rows (n, D), or None without users"""
    return np.stack([np.asarray(u["embeds"][key], np.float32).reshape(-1) for u in users]) if users else None


def request_arrays(states, medium, weights=False):
    """The arguments of `RecommenderModel.retrieve_request` for render.jl request states of one medium, one group per state: the
    users' "{medium}.retrieval" embeddings (n, D), their group ids, each user's list items as (medium, matchedid, status) in list
    order, and each state's selected items as (medium, matchedid) in order.  weights=True: then the two arrays of `state_weights`."""
    users, group, hist, sel = _users_and_selected(states, "retrieval")
    return (_embeds(users, f"{medium}.retrieval"), group, hist, sel) + (state_weights(states) if weights else ())


def retrieval(model, states, k=1024, coefs=None, search=None):
    """render.jl `retrieval(state)` on the device for a list of request states (`medium`, `items`, `users[*].embeds`,
    `users[*].user.items`), one group per state, on the tables of `load_retrieval_tables`: prior of the selected items, summed log
    soft-max of the users, relation / watched / selected / item-0 / unreleased masks, best first.  `coefs`: the registry's retrieval
    coefficient (adds n_users * log(coef), the order does not change; with user weights, sum of w_u * log(coef)).  Users and selected
    items may carry a "weight" (`state_weights`); a state may carry "texts" (`state_texts`), scored through `search` = {medium:
    SearchModel} and added to its prior.  Returns one (ids, scores) pair per state, ids 0-based medium-local, at most min(k, V_m, 8192)
    of them."""
    out = [None] * len(states)
    for m, idx in _by_medium(states, "retrieval: "):
        q, group, hist, sel, uw, sw = request_arrays([states[j] for j in idx], m, weights=True)
        Vm = model.config["vocab_sizes"][f"{m}_matchedid"]
        kk = min(int(k), Vm, 8192)
        with _texts(model, [states[j] for j in idx], search):
            ids, scores, counts = model.retrieve_request(q, m, kk, group=group, histories=hist, selected=sel, user_weights=uw,
                                                         selected_weights=sw)
        members = np.bincount(group, minlength=len(idx)) if uw is None else \
            np.bincount(group, weights=uw.astype(np.float64), minlength=len(idx))
        for g, j in enumerate(idx):
            n = int(counts[g])
            s = scores[g, :n]
            if coefs is not None:
                s = (s.astype(np.float64) + members[g] * np.log(float(np.asarray(coefs).reshape(-1)[0]))).astype(np.float32)
            out[j] = (ids[g, :n].copy(), s)
    return out


def _window_arrays(states, medium, weights=False):
    """`request_arrays` for states that may have no users: (queries or None, group ids, list items per user, selected items per state)"""
    users, group, hist, sel = _users_and_selected(states)
    return (_embeds(users, f"{medium}.retrieval"), group, hist, sel) + (state_weights(states) if weights else ())


def retrieval_window(model, states, windows, search=None):
    """Ranks [start, start + length) of render.jl `retrieval(state)` and its exact length (rsys_retrieve_window), for a list of request
    states with or without users: `retrieval`'s ordering without its cap of 8192 -- any start, at most 1024 ranks per call.  A state
    without users (compute.jl `/add_item`) is ordered by the item-similarity prior of its selected items alone.  `windows`: one
    (start, length) pair, or one per state.  Returns one (ids, scores, total) triple per state: the window's ids (0-based
    medium-local) and scores, best first -- fewer than `length` when the list ends inside the window, none when it starts past the end
    -- and the number of admissible items.  `search`: as in `retrieval`; a state without users is then ordered by prior + texts."""
    wins = [windows] * len(states) if np.ndim(windows) == 1 else list(windows)
    if len(wins) != len(states):
        raise ValueError(f"retrieval_window: {len(wins)} windows for {len(states)} states")
    for start, length in wins:
        if int(start) < 0 or not 1 <= int(length) <= MAX_ITEMS_TO_RANK:
            raise ValueError("retrieval_window: start >= 0 and 1 <= length <= 1024")
    out = [None] * len(states)
    for m, idx in _by_medium(states):
        q, group, hist, sel, uw, sw = _window_arrays([states[j] for j in idx], m, weights=True)
        with _texts(model, [states[j] for j in idx], search):
            ids, scores, counts, totals = model.retrieve_window(q, m, [int(wins[j][0]) for j in idx], [int(wins[j][1]) for j in idx],
                                                                group=group, n_groups=len(idx), histories=hist, selected=sel,
                                                                user_weights=uw, selected_weights=sw)
        for g, j in enumerate(idx):
            n = int(counts[g])
            out[j] = (ids[g, :n].copy(), scores[g, :n].copy(), int(totals[g]))
    return out


# ---------------------------------------------------------------- ranking and reranking (render.jl `ranking`, `reranking!`, `render`)
MAX_ITEMS_TO_RANK = 1024          # render.jl:449
RETRIEVAL_CAP = 8192              # candidates rsys_retrieve_request returns at most


def load_ranking_tables(model, relations):
    """Loads render.jl's "{m}.related" (a Julia-shaped SparseMatrixCSC dict or a 0-based CSC tuple / object, `julia_csc`) onto the
    device for `reranking`; a medium whose key is absent is left as it is.  The item-similarity embeddings come from
    `load_retrieval_tables`."""
    for m in (0, 1):
        if f"{m}.related" in relations:
            model.set_related(m, julia_csc(relations[f"{m}.related"]))


def _registry_coefs(registry, m):
    """(retrieval coefficient or None, rating coefficients or None, rating mean) as compute_retrieval / compute_ranking read them"""
    if registry is None:
        return None, None, 0.0
    rc = registry.get(f"{m}.retrieval.coefs")
    kc = registry.get(f"{m}.rating.coefs")
    rc = None if rc is None else float(np.asarray(rc).reshape(-1)[0])
    kc = None if kc is None else np.asarray(kc, np.float32).reshape(-1)[:2]
    mean = float(np.asarray(registry[f"{m}.rating_mean"])) if kc is not None else 0.0
    return rc, kc, mean


def rank_arrays(states, idxs, with_embeds=True, weights=False):
    """The per-user arguments of `RecommenderModel.rank_request` for render.jl states of one medium (one group per state, `idxs[g]` its
    candidates): queries (n, D) or None, group ids, r_masked (one row per user: its "{m}.ranking" values), list items (medium,
    matchedid, status) in list order -- every entry, duplicates and all statuses included -- and per group the penalties
    (decay, mmr_penalty, same_series_penalty, related_penalty) of `state["penalties"]`.  weights=True: then the two arrays of
    `state_weights` (the ranking reads the users' only)."""
    users, group, hist, _ = _users_and_selected(states, "ranking", selected=False)
    pen = [[float(st.get("penalties", {}).get(k, 0.0)) for k in ("decay", "mmr_penalty", "same_series_penalty", "related_penalty")]
           for st in states]
    q = rm = None
    if with_embeds:
        q, rm = [], []
        for u, g in zip(users, group):
            m = int(states[g]["medium"])
            q.append(np.asarray(u["embeds"][f"{m}.retrieval"], np.float32).reshape(-1))
            rm.append(np.asarray(u["embeds"][f"{m}.ranking"], np.float32).reshape(-1))
            if rm[-1].size != len(idxs[g]):
                raise ValueError(f"ranking: a user has {rm[-1].size} \"{m}.ranking\" values for {len(idxs[g])} candidates")
        q = np.stack(q)
    return (q, group, rm, hist, np.asarray(pen, np.float32).reshape(-1, 4)) + (state_weights(states) if weights else ())


def _by_medium(states, who=""):
    """[(medium, indices of its states)], media ascending; `who` starts the refusal's text"""
    out = {}
    for j, st in enumerate(states):
        m = int(st["medium"])
        if m not in (0, 1):
            raise ValueError(f"{who}medium must be 0 or 1")
        out.setdefault(m, []).append(j)
    return sorted(out.items())


def ranking(model, states, idxs, registry=None, search=None):
    """render.jl `ranking(state, idxs)` on the device for a list of states (one candidate array `idxs[j]` of 0-based medium-local ids
    per state): score = sum over the state's users, in order, of log(p_u[idxs]) + r_u, with p_u = coef * softmax(table_m . u) and
    r_u = c0 * rating_mean + c1 * "{m}.ranking" (compute_retrieval / compute_ranking; without registry coefficients p_u = softmax and
    r_u = "{m}.ranking").  Every user needs "{m}.retrieval" and "{m}.ranking" (the rating head at the candidates, `predict(...,
    "ranking")`) in its embeds.  A state's "texts" (`state_texts`, scored through `search` = {medium: SearchModel}) come first: w_t *
    log_softmax of the text at the candidates, no coefficient and no rating term.  Returns one float32 score array per state."""
    out = [None] * len(states)
    for m, js in _by_medium(states):
        sub, cand = [states[j] for j in js], [np.asarray(idxs[j]) for j in js]
        q, group, rm, hist, _, uw, _ = rank_arrays(sub, cand, weights=True)
        rc, kc, mean = _registry_coefs(registry, m)
        with _texts(model, sub, search):
            _, r = model.rank_request(q, m, cand, group=group, r_masked=rm, retrieval_coef=rc, rating_coefs=kc, rating_mean=mean,
                                      rerank=False, user_weights=uw)
        for g, j in enumerate(js):
            out[j] = r[g]
    return out


def reranking(model, states, idxs, r, partialk):
    """render.jl `reranking!(state, idxs, r, partialk)` on the device: per state the greedy min(partialk, n) picks under the MMR,
    same-series and related penalties of `state["penalties"]` (keys decay, mmr_penalty, same_series_penalty, related_penalty) from the
    tables of `load_retrieval_tables` (item similarity) and `load_ranking_tables` ("{m}.related").  `r`: one score array per state;
    `partialk`: an int or one per state.  Returns one array of picked ids (0-based medium-local, in pick order) per state."""
    pks = [int(partialk)] * len(states) if np.ndim(partialk) == 0 else [int(x) for x in partialk]
    out = [None] * len(states)
    for m, js in _by_medium(states):
        sub, cand = [states[j] for j in js], [np.asarray(idxs[j]) for j in js]
        _, group, _, hist, pen = rank_arrays(sub, cand, with_embeds=False)
        ids, _ = model.rank_request(None, m, cand, group=group, partialk=[pks[j] for j in js], penalties=pen, histories=hist,
                                    scores=[r[j] for j in js])
        for g, j in enumerate(js):
            out[j] = ids[g]
    return out


def page_window(n_retrieved, pagination):
    """render.jl:447-465 for one state: (start, stop) of the ranked slice of the retrieved list, (sidx, eidx) 1-based within it, or None
    when the page starts past the list.  max_items_to_rank = 1024 - 1024 % limit.  Deviation: render.jl throws a BoundsError when the
    ranked slice runs past the retrieved list; here it is clamped to it."""
    limit, offset = int(pagination["limit"]), int(pagination["offset"])
    if limit < 1 or offset < 0:
        raise ValueError("pagination: limit >= 1 and offset >= 0")
    mitr = MAX_ITEMS_TO_RANK - MAX_ITEMS_TO_RANK % limit
    sidx, eidx = offset + 1, offset + limit
    if sidx > n_retrieved:
        return None
    eidx = min(eidx, n_retrieved)
    page = (sidx - 1) // mitr
    start, stop = page * mitr, min((page + 1) * mitr, n_retrieved)
    return start, stop, sidx - start, eidx - start


def _penalties(st):
    p = st.get("penalties", {})
    return [float(p.get(k, 0.0)) for k in ("decay", "mmr_penalty", "same_series_penalty", "related_penalty")]


def render_items(model, states, pagination, search=None):
    """render.jl `render(state, pagination)` for states WITHOUT users (compute.jl:490-514 `/add_item`: pick a title, see similar
    titles) in one device call (rsys_render_items): `retrieval` is the item-similarity prior of the selected items with item 0, the
    selected and the unreleased items masked, `ranking` is zeros, `reranking!` runs on them under `state["penalties"]`.  `pagination`:
    {"offset", "limit"} or one per state.  Returns one (ids of the page, total) pair per state; total is the exact number of admissible
    items and every offset below it has a page.  A state's "texts" (`state_texts`, through `search` = {medium: SearchModel}) join the
    prior: "search for a phrase, get a reranked page" is a state with a text and no selected item."""
    pags = [pagination] * len(states) if isinstance(pagination, dict) else list(pagination)
    if len(pags) != len(states):
        raise ValueError(f"render_items: {len(pags)} paginations for {len(states)} states")
    gm, off, lim, pen, sel = [], [], [], [], []
    for st, pg in zip(states, pags):
        if st["users"]:
            raise ValueError("render_items: a state has users (render, render_users)")
        m, limit, offset = int(st["medium"]), int(pg["limit"]), int(pg["offset"])
        if m not in (0, 1):
            raise ValueError("medium must be 0 or 1")
        if not 1 <= limit <= MAX_ITEMS_TO_RANK or offset < 0:
            raise ValueError("pagination: 1 <= limit <= 1024 and offset >= 0")
        gm.append(m); off.append(offset); lim.append(limit)
        pen.append(_penalties(st))
        sel.append([(int(a["medium"]), int(a["matchedid"])) for a in st["items"]])
    if not states:
        return []
    with _texts(model, states, search):
        pages, totals = model.render_items(gm, off, lim, np.asarray(pen, np.float32).reshape(-1, 4), sel,
                                           selected_weights=state_weights(states)[1])
    return [(pages[g], int(totals[g])) for g in range(len(states))]


def render(model, states, pagination, registry=None, max_ranking_items=None, full_history=False, exact=False, trim=False, compact_top=False,
           search=None):
    """render.jl `render(state, pagination)` (lines 437-474) without the card rendering, for a list of states: `retrieval`, the page's
    slice of at most 1024 candidates, the ranking forward (`predict(..., "ranking")` in chunks of at most `max_ranking_items` candidates,
    default the model's S - S // 2; candidates are masked from each other, so chunking does not change the result of a user with a
    history -- with an EMPTY history the first candidate of every chunk carries mask id 0 and is seen by the chunk's others, so there
    the values depend on where the chunks are cut), then `ranking` + `reranking` in one device call with partialk = the page's last
    index.  `full_history=True`: the ranking forward is `predict_ranking_full` instead -- every user ranked on its newest S - 1 events
    (the reference's row) rather than the S // 2 - 1 that fit beside a chunk; `max_ranking_items` is then not used.  `pagination`:
    {"offset", "limit"} or one per state.  Returns one (ids of the page, total) pair per state.  Deviation: the ranked slice is
    clamped to the retrieved list (render.jl throws a BoundsError).  By default total = min(admissible items, 8192), the retrieval cap, a
    page past rank 8192 is empty and every state needs a user; both are closed by `exact=True` / `render_items`: the page's candidates
    then come from `retrieval_window`, so total is the number of admissible items and every offset below it has a page (ranking and
    reranking unchanged), and states without users go through `render_items` -- every state render.jl renders.  `trim=True`: the
    ranking forwards run trimmed (`predict(..., trim=True)` / `predict_ranking_full(..., trim=True)`).  `compact_top=True`: they run
    under rsys_serving_compact_top_set (`predict(..., compact_top=True)` / `predict_ranking_full(..., compact_top=True)`).  `search` =
    {medium: SearchModel}: the states' "texts" (`state_texts`) reach `retrieval` / `retrieval_window` and `ranking`."""
    if compact_top:
        with _compact_top(model):
            return render(model, states, pagination, registry, max_ranking_items, full_history, exact, trim, search=search)
    pags = [pagination] * len(states) if isinstance(pagination, dict) else list(pagination)
    if exact:
        for pg in pags:
            if not 1 <= int(pg["limit"]) <= MAX_ITEMS_TO_RANK or int(pg["offset"]) < 0:
                raise ValueError("pagination: 1 <= limit <= 1024 and offset >= 0")
        out = [None] * len(states)
        bare = [j for j, st in enumerate(states) if not st["users"]]
        for j, res in zip(bare, render_items(model, [states[j] for j in bare], [pags[j] for j in bare], search)):
            out[j] = res
        rest = [j for j, st in enumerate(states) if st["users"]]
        if rest:
            for j, res in zip(rest, _render_states(model, [states[j] for j in rest], [pags[j] for j in rest], registry, max_ranking_items,
                                                  full_history, True, trim, search)):
                out[j] = res
        return out
    return _render_states(model, states, pags, registry, max_ranking_items, full_history, False, trim, search)


def _render_states(model, states, pags, registry, max_ranking_items, full_history, exact, trim=False, search=None):
    """`render` for states with users; exact: the page's candidates are the window of `retrieval_window` instead of a slice of the top 8192"""
    S = model.config["max_sequence_length"]
    max_user_len = S // 2
    chunk = S - max_user_len if max_ranking_items is None else min(int(max_ranking_items), S - max_user_len)
    if chunk < 1:
        raise ValueError("render: max_ranking_items must be >= 1")
    out = [None] * len(states)
    work = []
    if exact:   # the ranked slice starts at a multiple of max_items_to_rank that the offset alone fixes: ask for exactly it
        mitr = [MAX_ITEMS_TO_RANK - MAX_ITEMS_TO_RANK % int(pg["limit"]) for pg in pags]
        windows = retrieval_window(model, states, [(int(pg["offset"]) // k * k, k) for pg, k in zip(pags, mitr)], search)
    else:
        retrieved = retrieval(model, states, k=RETRIEVAL_CAP, coefs=None, search=search)
    for j, st in enumerate(states):
        if exact:
            ids, _, total = windows[j]
            win = page_window(total, pags[j])
        else:
            ids = retrieved[j][0]
            total = int(ids.size)
            win = page_window(total, pags[j])
            if win is not None:
                ids = ids[win[0]:win[1]]
        if win is None:
            out[j] = (np.zeros(0, np.int32), total)
            continue
        work.append((j, ids, win[2], win[3], total))
    for m, js in _by_medium([states[w[0]] for w in work]) if work else []:
        items = [work[i] for i in js]
        sub = [states[w[0]] for w in items]
        for st, w in zip(sub, items):         # the ranking forward: "{m}.ranking" at the page's candidates, per user
            cand = w[1]
            if full_history:
                reqs = [dict(u["user"], ranking_items=[int(x) for x in cand]) for u in st["users"]]
                for u, r in zip(st["users"], predict_ranking_full(model, reqs, m, trim=trim)):
                    u.setdefault("embeds", {})[f"{m}.ranking"] = np.asarray(r[f"{m}.ranking"], np.float32)
                continue
            for u in st["users"]:
                vals = []
                for c0 in range(0, cand.size, chunk):
                    req = dict(u["user"], ranking_items=[int(x) for x in cand[c0:c0 + chunk]])
                    vals += predict(model, [req], "ranking", m, max_user_len, S - max_user_len, trim=trim)[0][f"{m}.ranking"]
                u.setdefault("embeds", {})[f"{m}.ranking"] = np.asarray(vals, np.float32)
        cand = [w[1] for w in items]
        q, group, rm, hist, pen, uw, _ = rank_arrays(sub, cand, weights=True)
        rc, kc, mean = _registry_coefs(registry, m)
        with _texts(model, sub, search):
            ids, _ = model.rank_request(q, m, cand, group=group, r_masked=rm, partialk=[w[3] for w in items], penalties=pen, histories=hist,
                                        retrieval_coef=rc, rating_coefs=kc, rating_mean=mean, user_weights=uw)
        for g, w in enumerate(items):
            out[w[0]] = (ids[g][w[2] - 1:w[3]], w[4])
    return out


# ---------------------------------------------------------------- a page from raw histories in one device call (rsys_render_request)
_ROW_COLS = _INT_COLS + ("time", "rating", "progress")


def _fill_row(d, row, seq, nh, who, num_items_0, ranking, c0=0):
    """row `row` of the ten arrays from the token sequence `seq` (nh history tokens first), exactly as `build_batch` fills the row of a
    one-user request: userid 1, history positions 0..nh-1 and mask id 0, appended tokens at position nh with their own mask id.
    `c0`: the column the sequence starts at (a segment of a packed row; positions and mask ids stay relative to it)"""
    L = len(seq)
    at = slice(c0, c0 + L)
    d["userid"][row, at] = 1
    d["gender"][row, at] = 0 if who["gender"] is None else who["gender"] + 1
    d["source"][row, at] = who["source"]
    d["time"][row, at] = [e["history_max_ts"] for e in seq]
    d["rope_input_pos"][row, at] = np.minimum(np.arange(L), nh)
    if ranking:
        d["token_mask_ids"][row, c0 + nh:c0 + L] = np.arange(nh, L)
    d["matchedid"][row, at] = [e["matchedid"] + (num_items_0 if e["medium"] == 1 else 0) for e in seq]
    d["status"][row, at] = [e["status"] for e in seq]
    d["rating"][row, at] = [e["rating"] for e in seq]
    d["progress"][row, at] = [e["progress"] for e in seq]


def _empty_rows(n, width):
    d = {k: np.zeros((n, width), np.int32) for k in _INT_COLS}
    d["time"] = np.zeros((n, width), np.float64)
    d["rating"] = np.zeros((n, width), np.float32)
    d["progress"] = np.zeros((n, width), np.float32)
    return d


def render_row_plan(n_candidates, nh, S):
    """Reference statement (tests and documentation; the library plans its rows itself): the ranking rows rsys_render_request runs for one user of a group whose page window holds `n_candidates` candidates: one
    (first candidate, candidates, action tokens within the row) triple per chunk of at most S - S // 2 candidates; none for an
    empty window.  The action token of candidate j of a chunk is 2 (nh + j) + 1 (`_selected_tokens`)."""
    chunk = S - S // 2
    return [(c0, min(chunk, n_candidates - c0), 2 * (nh + np.arange(min(chunk, n_candidates - c0))) + 1)
            for c0 in range(0, int(n_candidates), chunk)]


def render_pack(states, pagination, S, num_items_0, registry=None, adapter_slots=None, full_history=False):
    """The arguments of `RecommenderModel.render_request` for render.jl request states (the states `render` takes; users need no
    "embeds"): every history is tokenised and projected once; from it come the user's retrieval row (`build_batch([user], "retrieval")`:
    the newest S - 1 tokens + the query token), the history part of its ranking rows (the first nh columns of `build_batch([user],
    "ranking")`: the newest S // 2 - 1 tokens) with the descriptor (nh, userid, gender, source) and timestamp the device completes them
    from, its list items, and per state the selected items, penalties, pagination and medium.  `full_history=True`: the arguments of
    `RecommenderModel.render_request_full` instead -- no prefix arrays, and the descriptor's first entry is n_hist = len(hr), the history
    columns of the retrieval row (the device cuts the cache's store rows from them).  When a user or a selected item carries a
    "weight", the dict also holds `user_weights` / `selected_weights` (`state_weights`); without any it has no such keys."""
    pags = [pagination] * len(states) if isinstance(pagination, dict) else list(pagination)
    if len(pags) != len(states):
        raise ValueError(f"render_users: {len(pags)} paginations for {len(states)} states")
    users, group = [], []
    gm, off, lim, pen, sel = [], [], [], [], []
    for g, st in enumerate(states):
        m = int(st["medium"])
        if m not in (0, 1):
            raise ValueError("medium must be 0 or 1")
        if not st["users"]:
            raise ValueError("render_users: every state needs at least one user")
        limit, offset = int(pags[g]["limit"]), int(pags[g]["offset"])
        if limit < 1 or offset < 0:
            raise ValueError("pagination: limit >= 1 and offset >= 0")
        gm.append(m); off.append(offset); lim.append(limit)
        p = st.get("penalties", {})
        pen.append([float(p.get(k, 0.0)) for k in ("decay", "mmr_penalty", "same_series_penalty", "related_penalty")])
        sel.append([(int(a["medium"]), int(a["matchedid"])) for a in st["items"]])
        for u in st["users"]:
            users.append(u["user"]); group.append(g)
    n = len(users)
    P = max(S // 2 - 1, 0)
    rows, prefix = _empty_rows(n, S), _empty_rows(n, P)
    tok = np.zeros(n, np.int32)
    desc = np.zeros((n, 4), np.int32)
    ts = np.zeros(n, np.float64)
    hist = []
    for i, user in enumerate(users):
        h = project(tokenize(user["items"]))                      # once per user
        hr = h[-(S - 1):] if len(h) > S - 1 else h
        hk = (h[-P:] if len(h) > P else h) if P else []
        who = user["user"]
        _fill_row(rows, i, hr + [make_item(user["timestamp"])], len(hr), who, num_items_0, False)
        _fill_row(prefix, i, hk, len(hk), who, num_items_0, True)
        tok[i] = 2 * len(hr)
        desc[i] = (len(hr) if full_history else len(hk), 1, 0 if who["gender"] is None else who["gender"] + 1, who["source"])
        ts[i] = user["timestamp"]
        hist.append([(int(x["medium"]), int(x["matchedid"]), int(x["status"])) for x in user["items"]])
    have, coefs = np.zeros(2, np.int32), np.zeros((2, 4), np.float32)
    for m in (0, 1):
        rc, kc, mean = _registry_coefs(registry, m)
        if rc is not None:
            have[m] |= 1; coefs[m, 0] = rc
        if kc is not None:
            have[m] |= 2; coefs[m, 1:3] = kc; coefs[m, 3] = mean
    slots = None
    if adapter_slots:
        slots = [adapter_slots[f"{m}.{task}"] for m in (0, 1) for task in ("retrieval", "ranking")]
    out = dict(group_medium=gm, offsets=off, limits=lim, penalties=np.asarray(pen, np.float32).reshape(-1, 4), group=group,
               retrieval_rows=rows, retrieval_token=tok, ranking_prefix=prefix, prefix_stride=P, user_desc=desc, user_ts=ts,
               adapter_slots=slots, histories=hist, selected=sel, coef_have=have, coefs=coefs)
    if full_history:
        del out["ranking_prefix"], out["prefix_stride"]
    uw, sw = state_weights(states)
    if uw is not None or sw is not None:
        out.update(user_weights=uw, selected_weights=sw)
    return out


def render_full_plan(n_hist, n_cand, S, max_rows):
    """Reference statement (tests and documentation; the library plans its rows itself): the ranking forwards rsys_render_request_full
    runs for users -- in r_masked order: the users of medium-0 groups with a page, then those of medium 1 -- with `n_hist[i]` history
    events and `n_cand[i]` >= 1 candidates.  Returns (waves, empty): `waves` = `rank_cache_plan` over the users with a history (user
    indices are positions in that sub-list), `empty` = the assembled rows of the others as (user, first candidate, candidates), one per
    `render_row_plan(n, 0, S)` chunk, users in order, which run in forwards of at most `max_rows` rows after the cached waves."""
    hist = [i for i, h in enumerate(n_hist) if h >= 1]
    waves = rank_cache_plan([n_hist[i] for i in hist], [n_cand[i] for i in hist], S, max_rows)
    waves = [([(hist[u], sl, nh) for u, sl, nh in store], [[(hist[u], sl, c0, n, nh) for u, sl, c0, n, nh in b] for b in batches])
             for store, batches in waves]
    empty = [(i, c0, n) for i, h in enumerate(n_hist) if h < 1 for c0, n, _ in render_row_plan(n_cand[i], 0, S)]
    return waves, empty


def render_full_forwards(n_hist, n_cand, S, max_rows, pack_store=False, slots=None):
    """(store forwards, candidate forwards, empty-history chunk forwards) of `render_full_plan`: what the library reports as "forwards.full".
    `pack_store=True`: what it reports under rsys_serving_pack_ranking_set -- waves of `slots` users with a history (the model's reserved
    cache slots; default `max_rows`), each wave's store stage planned as `rank_cache_pack_plan` plans it, its candidate rows (chunks of at
    most S, one per row) in forwards of `max_rows` rows."""
    if not pack_store:
        waves, empty = render_full_plan(n_hist, n_cand, S, max_rows)
        return len(waves), sum(len(b) for _, b in waves), -(-len(empty) // max_rows)
    slots = max_rows if slots is None else int(slots)
    hist = [i for i, h in enumerate(n_hist) if h >= 1]
    empty = [c for i, h in enumerate(n_hist) if h < 1 for c in render_row_plan(n_cand[i], 0, S)]
    store = cands = 0
    for w0 in range(0, len(hist), slots):
        wave = hist[w0:w0 + slots]
        store += len(_plan_segments([int(n_hist[i]) for i in wave], S, max_rows))
        cands += -(-sum(-(-int(n_cand[i]) // S) for i in wave) // max_rows)
    return store, cands, -(-len(empty) // max_rows)


def render_full_store_rows(n_hist, S, max_rows, slots=None):
    """The packed store forwards of `render_full_forwards(pack_store=True)` as the library reports them in "forward_rows": [(rows, row_len)]
    in run order, for the users with a history."""
    slots = max_rows if slots is None else int(slots)
    hist = [int(h) for h in n_hist if h >= 1]
    return [(1 + max(r for _, r, _ in placed), row_len) for w0 in range(0, len(hist), slots)
            for row_len, placed in _plan_segments(hist[w0:w0 + slots], S, max_rows)]


def render_users(model, states, pagination, registry=None, full_history=False, trim=False, pack=False, pack_ranking=False, compact_top=False,
                 search=None):
    """`render` from raw histories in ONE device call (rsys_render_request): the same states, but users need no "embeds" -- the
    retrieval forward, `retrieval`, the page window, the ranking forward (every chunk row of every user, both media, in waves of the
    model's max_rows) and `ranking` + `reranking` run back to back on the device; only the pages and the totals come back.  A model built
    by `get_models` runs every row with the adapter of its "{medium}.{task}"; a plain model runs the base.  Returns one (ids of the
    page, total) pair per state, as `render`.  `full_history=True` (rsys_render_request_full): the ranking forward of
    `render(..., full_history=True)` inside the same call -- every user ranked on its newest S - 1 events through the per-user K/V cache,
    whose store rows the device cuts from the retrieval rows it already holds; no ranking prefix is built or uploaded.
    `trim=True` (rsys_serving_trim_set for the length of the call): every forward of the pipeline runs at the length of its longest live
    row in whole 64-token tiles; waves, chunks, slots and outputs are unchanged.
    `pack=True` (rsys_serving_pack_set and, as packing implies trimming, rsys_serving_trim_set for the length of the call): the
    retrieval stage runs several users per row (`pack_plan`'s layout); the ranking stages are the trimmed ones.
    `pack_ranking=True` (rsys_serving_pack_ranking_set for the length of the call; `full_history=True` only): the K/V-cache store rows
    hold several users, in waves of up to the model's reserved cache slots (`rank_cache_pack_plan`'s store stage); pages and totals are
    unchanged.
    `compact_top=True` (rsys_serving_compact_top_set for the length of the call): every forward of the pipeline runs its last layer only
    where its outputs are read; scores agree with the dense pipeline to rounding, so two items closer than that may swap places.
    `search` = {medium: SearchModel}: the states' "texts" (`state_texts`) reach the retrieval and the ranking stage of their medium."""
    if compact_top:
        with _compact_top(model):
            return render_users(model, states, pagination, registry, full_history, trim, pack, pack_ranking, search=search)
    if not states:
        return []
    if pack_ranking and not full_history:
        raise ValueError("render_users: pack_ranking packs the K/V-cache store rows, which only full_history=True runs")
    trim = trim or pack
    args = render_pack(states, pagination, model.config["max_sequence_length"], model.config["vocab_sizes"]["0_matchedid"], registry,
                       getattr(model, "adapter_slots", None), full_history)
    before = model.serving_trim if trim else False
    if trim:
        model.serving_trim = True
    if pack:
        model.serving_pack = True
    if pack_ranking:
        model.serving_pack_ranking(True)
    try:
        with _texts(model, states, search):
            pages, totals = (model.render_request_full if full_history else model.render_request)(**args)
    finally:
        if trim:
            model.serving_trim = before
        if pack:
            model.serving_pack = False
        if pack_ranking:
            model.serving_pack_ranking(False)
    return [(pages[g], int(totals[g])) for g in range(len(states))]
