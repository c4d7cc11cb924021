"""numpy side of the retrieval selection tests (test_gpu_retrieve.py, test_gpu_retrieve_select.py, test_retrieve_select_host.py): the score
populations, the stable-sort reference of rsys_op_topk / rsys_op_topk_window, a restatement of the windowed radix select's two rank
bounds (what the hook's `bounds` must hold), the named windows the tests ask for, and a float32 restatement of the log-sum-exp kernels'
fold order.  No GPU is needed to import or run anything here."""
import numpy as np

RT_WIN = 1024
LSE_SPLIT, LSE_THREADS = 64, 256

# bit patterns 0x40000000 + c: neighbouring blocks straddle every 8-bit digit boundary of the key, and the lower neighbour of each
# boundary is the all-ones key that a between-form threshold (prefix - 1) takes
DIGIT_EDGES = np.array([0, 0xff, 0x100, 0xffff, 0x10000, 0xffffff, 0x1000000], np.int64)
_EDGE_P_SMALL = np.array([0.25, 0.10, 0.20, 0.05, 0.15, 0.10, 0.15])
_EDGE_P_LARGE = np.array([0.30, 0.004, 0.25, 0.002, 0.222, 0.002, 0.22])   # blocks of a few hundred between blocks of tens of thousands


def _expect_topk(row, k):
    ids = np.arange(row.size)
    ok = ~np.isnan(row) & (row > -np.inf)
    order = np.lexsort((ids[ok], -row[ok].astype(np.float64)))
    sel = ids[ok][order][:k]
    vals = row[sel] + np.float32(0.0)            # -0.0 comes back as +0.0
    return sel.astype(np.int32), vals.astype(np.float32)


def _rows(kind, rows, V, rng):
    if kind == "random":
        return rng.standard_normal((rows, V)).astype(np.float32) * 4 - 10
    if kind == "equal":
        return np.full((rows, V), -3.25, np.float32)
    if kind == "ulp":      # a handful of neighbouring floats: every digit pass runs, long runs of ties
        base = np.float32(-7.5).view(np.int32)
        return (base + rng.integers(0, 5, (rows, V))).astype(np.int32).view(np.float32)
    if kind == "zeros":    # +-0.0 mixed with a few values around them
        x = np.where(rng.random((rows, V)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        x[rng.random((rows, V)) < 0.05] = 1e-30
        x[rng.random((rows, V)) < 0.05] = -1e-30
        return x
    if kind == "special":  # -inf and NaN sprinkled in; the last row all -inf
        x = rng.standard_normal((rows, V)).astype(np.float32)
        x[rng.random((rows, V)) < 0.3] = -np.inf
        x[rng.random((rows, V)) < 0.1] = np.nan
        x[rng.random((rows, V)) < 0.01] = np.inf
        x[-1] = -np.inf
        return x
    if kind == "digit_edges":   # row r: positive (r % 3 == 0), negated (keys of negative floats are ~u; r % 3 == 1), both signs (r % 3 == 2)
        p = _EDGE_P_SMALL if V < 20000 else _EDGE_P_LARGE
        c = rng.choice(DIGIT_EDGES, size=(rows, V), p=p / p.sum())
        x = (0x40000000 + c).astype(np.uint32).view(np.float32).copy()
        for r in range(rows):
            if r % 3 == 1:
                x[r] = -x[r]
            elif r % 3 == 2:
                neg = rng.random(V) < 0.5
                x[r, neg] = -x[r, neg]
        return x
    raise AssertionError(kind)


# ---------------------------------------------------------------- the ordering and its windows
def full_order(row):
    """ids of the admissible entries (not NaN, > -inf) by descending value, ties by ascending id."""
    ids = np.arange(row.size)
    ok = ~np.isnan(row) & (row > -np.inf)
    order = np.lexsort((ids[ok], -row[ok].astype(np.float64)))
    return ids[ok][order].astype(np.int32)


def expect_window(row, order, start, length):
    """(ids [1024], vals [1024], count, total) of the window [start, start + length) of `order` with -1 / -inf padding."""
    total = order.size
    count = int(np.clip(total - start, 0, length))
    ids = np.full(RT_WIN, -1, np.int32)
    vals = np.full(RT_WIN, -np.inf, np.float32)
    if count:
        sel = order[int(start):int(start) + count]
        ids[:count] = sel
        vals[:count] = row[sel] + np.float32(0.0)
    return ids, vals, count, total


def score_keys(row):
    """the order-preserving uint32 key of every score (score_key, common.hpp): 0 = NaN / -inf, -0.0 merged into +0.0."""
    x = np.ascontiguousarray(row, np.float32) + np.float32(0.0)
    u = x.view(np.uint32).astype(np.int64)
    key = np.where(u & 0x80000000, ~u & 0xffffffff, u | 0x80000000)
    key[np.isnan(x) | ~(x > -np.inf)] = 0
    return key


def select_bound(keys, c):
    """The pair (T, need) win_select_step_kernel resolves the rank bound c to: the top-c set is every key above T plus the first `need`
    keys equal to T by ascending id.  keys: int64 array of uint32 keys, 0 = excluded."""
    keys = keys[keys != 0]
    adm = keys.size
    if c <= 0:
        return 0xffffffff, 0
    if c >= adm:
        return 0, 0
    prefix, rmask, need = 0, 0, int(c)
    for p in range(4):
        shift = 24 - 8 * p
        open_ = keys[(keys & rmask) == prefix]
        cb = np.bincount((open_ >> shift) & 0xff, minlength=256)
        cum, b = 0, 255
        while b > 0:
            if cum + cb[b] >= need:
                break
            cum += cb[b]
            b -= 1
        prefix |= b << shift
        rmask |= 0xff << shift
        need -= cum
        if shift == 0:
            return prefix, need
        if cb[b] == need:           # the bin is taken whole: between two keys
            return (prefix if prefix else 1) - 1, 0
    raise AssertionError


def expect_bounds(row, start, length):
    """[[T_end, need_end], [T_start, need_start]] as the hook's `bounds` row holds them (T as int32 bits)."""
    keys = score_keys(row)
    adm = int((keys != 0).sum())
    lo = min(int(start), adm)
    stop = lo + int(np.clip(adm - start, 0, length))
    out = np.array([select_bound(keys, stop), select_bound(keys, lo)], np.int64)
    return out.astype(np.uint32).view(np.int32)


def is_between_form(T, need):
    return need == 0 and (T & 0xffffffff) not in (0, 0xffffffff)


WINDOW_NAMES = ["first", "inside_largest", "block_start", "block_end", "real_key_at_T", "two_blocks", "three_blocks", "last_five",
                "at_total", "past_total", "far_past", "exactly_1024_left", "only_1023_left"]


def named_windows(row, order):
    """{name: (start, len)} of the windows the select tests name, chosen from the tie-block edges of the row's ordering; a name is
    missing where the row has no such window (too few blocks or ranks)."""
    total = order.size
    W = {"at_total": (total, 7), "past_total": (total + 100, 1), "far_past": (2 ** 40, 1024)}
    if total == 0:
        return W
    W["first"] = (0, 1)
    W["last_five"] = (max(total - 5, 0), 1024)
    if total >= 1024:
        W["exactly_1024_left"] = (total - 1024, 1024)
    if total >= 1023:
        W["only_1023_left"] = (total - 1023, 1024)
    keys = score_keys(row)
    skeys = keys[order]
    edges = np.flatnonzero(np.diff(skeys)) + 1                       # first rank of every block but the first
    first = np.concatenate([[0], edges])                             # first rank of block j
    size = np.diff(np.concatenate([first, [total]]))
    big = int(np.argmax(size))
    if size[big] >= 3:                                               # strictly inside: both bounds exact on one key, need_start > 0
        W["inside_largest"] = (int(first[big]) + 1, int(min(size[big] - 2, RT_WIN)))
    between = {}                                                     # block j -> the start bound at its first rank has the between form
    probe = range(1, first.size) if first.size <= 41 else np.unique(np.linspace(1, first.size - 1, 40).astype(np.int64)).tolist()
    for j in probe:                                                  # (every block of a tied population; 40 of them where all scores differ)
        T, need = select_bound(keys, int(first[j]))
        if need == 0:
            between[j] = T
    for j in between:                                                # a window from a block's first rank to the middle of the next block or itself
        W["block_start"] = (int(first[j]), int(min(max(size[j] // 2, 1), RT_WIN)))
        break
    for j in between:                                                # ... ending at the last rank of block j - 1, from inside it
        n = int(min(max(size[j - 1] // 2, 1), RT_WIN))
        W["block_end"] = (int(first[j]) - n, n)
        break
    for j, T in between.items():                                     # a real key equal to the between-form T; the window ends inside its block
        if T == skeys[first[j]] and size[j] >= 2:
            W["real_key_at_T"] = (int(first[j]), int(min(size[j] - 1, RT_WIN)))
            break
    for j in range(first.size - 1):                                  # inside block j to inside block j + 1: nothing strictly between
        if size[j] >= 2 and size[j + 1] >= 2:
            a, b = int(min(size[j] - 1, 3)), int(min(size[j + 1] - 1, 3))
            W["two_blocks"] = (int(first[j + 1]) - a, a + b)
            break
    for j in range(first.size - 2):                                  # inside block j, all of j + 1 .., into a later block
        if size[j] >= 2 and size[j + 1] + 2 <= RT_WIN:
            a = int(min(size[j] - 1, 3))
            room = RT_WIN - a
            stop = int(min(first[j + 1] + room, total))
            if skeys[stop - 1] != skeys[first[j + 1]]:                # reaches a third block
                W["three_blocks"] = (int(first[j + 1]) - a, stop - (int(first[j + 1]) - a))
                break
    return W


# ---------------------------------------------------------------- log-sum-exp
LSE_KINDS = ["random", "equal", "ascending", "descending", "spike", "near_88", "near_m100", "inf_stripe"]
LSE_VS = [1, 2, 37, 63, 64, 65, 129, 16384, 16385, 119999]
LSE_ROWS = [1, 3, 257]


def lse_rows(kind, rows, V, rng):
    x = rng.standard_normal((rows, V)).astype(np.float32) * 2 - 10       # N(0, 4) - 10
    if kind == "random":
        return x
    if kind == "equal":
        return np.full((rows, V), -3.25, np.float32)
    if kind == "ascending":        # a rescale on every element
        return np.sort(x, axis=1)
    if kind == "descending":
        return np.sort(x, axis=1)[:, ::-1].copy()
    if kind == "spike":            # one element 90 above the rest
        x[np.arange(rows), rng.integers(0, V, rows)] += np.float32(90)
        return x
    if kind == "near_88":          # expf overflows unless the max is subtracted
        return (x + np.float32(98)).astype(np.float32)
    if kind == "near_m100":
        return (x - np.float32(90)).astype(np.float32)
    if kind == "inf_stripe":       # the first 3000 entries (half the row where it is shorter) are -inf, the rest finite
        x[:, :3000 if V > 3000 else V // 2] = -np.inf
        return x
    raise AssertionError(kind)


def lse_case(V, rows):
    """(z [rows][V], kind of every row): row r is of kind LSE_KINDS[r % 8], so one call of `rows` rows holds every kind it has room for."""
    rng = np.random.default_rng(1000 * rows + V)
    kinds = [LSE_KINDS[r % len(LSE_KINDS)] for r in range(rows)]
    if rows == 1:
        kinds = [LSE_KINDS[V % len(LSE_KINDS)]]
    z = np.empty((rows, V), np.float32)
    for k in LSE_KINDS:
        sel = [r for r, kk in enumerate(kinds) if kk == k]
        if sel:
            z[sel] = lse_rows(k, len(sel), V, rng)
    return z, kinds


def lse_fp64(z):
    z = z.astype(np.float64)
    m = z.max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = m + np.log(np.exp(z - m[:, None]).sum(axis=1))
    out[np.isneginf(m)] = -np.inf
    return out


def _fold(m, s, m2, s2):
    """lse_fold: (m, s) <- the merge of two (max, sum exp(. - max)) pairs, float32; both maxima -inf: (m, s) is left as it is."""
    mx = np.maximum(m, m2)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.where(np.isneginf(m), np.float32(0), s * np.exp(m - mx, dtype=np.float32))
        b = np.where(np.isneginf(m2), np.float32(0), s2 * np.exp(m2 - mx, dtype=np.float32))
    keep = np.isneginf(mx)
    return np.where(keep, m, mx).astype(np.float32), np.where(keep, s, (a + b).astype(np.float32)).astype(np.float32)


def lse_restated(z):
    """float32 log-sum-exp of every row in the kernels' order: 64 slices [V p / 64, V (p + 1) / 64), 256 lanes each taking every 256th
    element with an online max / rescale, lanes folded by xor 32..1 inside a wave, the four waves in order, then the slices in order."""
    z = np.ascontiguousarray(z, np.float32)
    rows, V = z.shape
    P, T = LSE_SPLIT, LSE_THREADS
    lo = (V * np.arange(P, dtype=np.int64)) // P
    hi = (V * (np.arange(P, dtype=np.int64) + 1)) // P
    m = np.full((rows, P, T), -np.inf, np.float32)
    s = np.zeros((rows, P, T), np.float32)
    stripes = int((hi - lo).max() + T - 1) // T
    for j in range(stripes):
        idx = lo[:, None] + j * T + np.arange(T)[None, :]                  # [P][T]
        live = idx < hi[:, None]
        x = z[:, np.where(live, idx, 0)]                                   # [rows][P][T]
        with np.errstate(invalid="ignore", over="ignore"):
            up = x > m
            s_up = np.where(np.isneginf(m), np.float32(0), s * np.exp(m - x, dtype=np.float32)) + np.float32(1)
            s_dn = s + np.exp(x - m, dtype=np.float32)
        ns = np.where(up, s_up, s_dn).astype(np.float32)
        nm = np.where(up, x, m)
        m = np.where(live[None], nm, m)
        s = np.where(live[None], ns, s)
    lane = np.arange(T)
    for o in (32, 16, 8, 4, 2, 1):
        m, s = _fold(m, s, m[:, :, lane ^ o], s[:, :, lane ^ o])
    M, S = m[:, :, 0], s[:, :, 0]
    for w in range(1, T // 64):
        M, S = _fold(M, S, m[:, :, 64 * w], s[:, :, 64 * w])
    fm = np.full(rows, -np.inf, np.float32)
    fs = np.zeros(rows, np.float32)
    for p in range(P):
        fm, fs = _fold(fm, fs, M[:, p], S[:, p])
    with np.errstate(divide="ignore", invalid="ignore"):
        return (fm + np.log(fs, dtype=np.float32)).astype(np.float32)


# Worst |lse_restated - fp64| per kind of row over LSE_VS x LSE_ROWS (test_retrieve_select_host.py measures and bounds each; the figures it
# printed are in the comments).  The GPU tolerance (test_gpu_retrieve_lse.py) is 4 x the largest of them: expf and logf of the device
# differ from numpy's by a few ulp per term.  An ulp of the result is 9.5e-7 around 10 and 7.6e-6 around 100, which separates the kinds.
LSE_RESTATED_ERR = {
    "random": 4.9e-7,       # measured 4.863e-07
    "equal": 3.8e-7,        # 3.787e-07
    "ascending": 4.9e-7,    # 4.842e-07
    "descending": 6.0e-7,   # 5.975e-07
    "spike": 0.0,           # 0: the other terms are below half an ulp of 1, the result is the spike itself in fp32 and in fp64
    "near_88": 4.1e-6,      # 4.097e-06
    "near_m100": 4.0e-6,    # 3.972e-06
    "inf_stripe": 4.8e-7,   # 4.767e-07
}
