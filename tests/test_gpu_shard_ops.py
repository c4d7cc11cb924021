"""GPU: the kernels of the row-sharded table (csrc/shard.hip), one launcher at a time through their C-ABI hooks (rsys_op_vp_ce, rsys_op_ss,
rsys_op_shard_rows in rsys_debug.h), against the float64 restatements of tests/_shard_np.py on the same (storage-rounded) inputs.  The hooks
hold no collective and no GEMM: the logits are an input, and what the model all-reduces between two stages this file reduces on the host
(max exactly, sums in fp32 in rank order), so "W ranks" are W calls with each rank's column range.

Bounds are derived by the rules of test_gpu_row_kernels.py (u = 2^-24): an fp32 result is within c u of the fp64 value scaled by the
magnitudes that went into it, c counting the roundings of the longest chain; a bf16-stored result within one bf16 ulp of the fp64 value, plus
the fp32 bound where it is a cancellation.  Integer outputs, copies, gathers and a + b row adds are compared bit for bit.  The counts:

  local sum-exp (vp_stats, ss_stats), relative: 7 L + 6 R + 24.  A thread's chain has L elements (vp: E ceil(ceil(Vloc / E) / 256) with E
    elements per 16-byte load; ss: ceil(n_tot / 256)); each costs an __expf (1 ulp = 2) and an addition (3) and may rescale the running
    sum first (another __expf, a product, the + 1: 4).  An __expf argument a = x - m is rounded twice (the subtraction, the product with
    log2 e): 2 u |a| relative in the result.  With R = the row's spread max - min: the terms' arguments are <= R (2 R), the arguments of
    a chain's rescales telescope to <= R (2 R), and so is the argument of the last rescale to the workgroup's maximum (2 R).  24: that
    last rescale (4) and the sum over the workgroup, a 6-level wave tree and the 16 wave partials in any order (6 + 14).
  sampled classes enter as y = x + __logf(s_j): 4 u log s_j for the logarithm (v_log 1 ulp = 2 u, the product with ln 2 and that
    constant 2 u) and u |y| for the addition = dy; the local maximum is within dy, the local sum relative to it within 2 dy more.
  the rebase to the global maximum, relative: 4 + 2 D (D = gmax - lmax: a subtraction, one __expf whose argument carries D u, a product).
  W additions on the host in fp32: W.
  lse = gmax + logf(S): the relative error of S, 2 u |log S| for logf (1 ulp), 2 u |lse| for the addition (as _ce_ref counts it).
    The sampled form's S = __expf(tl - gmax) + sneg costs 4 + 2 |tl - gmax| more.
  loss term (lse - tl) lw: e_lse |lw| + 2 u |term|; a rank's loss: its rows' terms, rows + 1 roundings of the magnitudes' sum.
  dlogit = coef (exp(x - lse) - onehot) [s_j]: p (e_lse + 2 u |x - lse| + 3 u) + 2^-125 (a probability below the smallest normal fp32 may
    flush to zero), times |coef| [s_j], plus 3 u |result| (4 u with the stratum weight's product).
  ss_target_logit: a lane's chain of ceil(D / 64) multiply-adds (2 each) and the 6-level wave tree: 2 ceil(D / 64) + 6.
  ss_target_grad: class row = prefill + k terms: k products and k additions in any order (atomics) or a chain of k multiply-adds and one
    addition (ordered): 2 k + 2 of the magnitudes' sum; the selected row = prefill + one product: 2.
"""
import ctypes as C

import numpy as np
import pytest

import _shard_np as sn
from test_gpu_row_kernels import BF16, DTYPES, F32, GUARD, SENT, U, Dev, _lib, _ok, bf16_ulp, storage

pytestmark = pytest.mark.gpu

ISENT = -777
NEG = np.float32(-3.0e38)
RATIO = {}          # kernel -> largest error / bound of the checks that ran (reported when the module is done; DESIGN.md quotes it)


def note(kernel, err, bound):
    """assert err <= bound element by element, in the positive form: a NaN in either (a kernel that read a NaN prefill, an overflow in
    the reference) fails; and record the largest error / bound (inf for such an element)"""
    err = np.asarray(err, np.float64); bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    ok = err <= bound
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    worst = float(r.max()) if r.size else 0.0
    RATIO[kernel] = max(RATIO.get(kernel, 0.0), worst)
    assert ok.all(), (kernel, worst, np.unravel_index(np.argmax(r), r.shape), float(err.ravel()[np.argmax(r)]))


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    """after the module's tests: the largest error / bound per kernel among the checks that ran (read it with -s)"""
    yield
    for k in sorted(RATIO):
        print(f"RATIO {k}: {RATIO[k]:.3f}")


class SDev(Dev):
    def puti(self, arr):
        return self.put(np.asarray(arr, np.int32))

    def geti(self, p, shape):
        n = int(np.prod(shape))
        h = np.empty(n + GUARD, np.int32)
        assert self.L.rsys_dev_d2h(h.ctypes.data, p, h.nbytes) == 0
        assert np.all(h[n:] == -12345), "write past the end of the buffer"
        return h[:n].reshape(shape)


@pytest.fixture
def dev():
    d = SDev()
    yield d
    d.free()


def f(x):
    return C.c_float(float(x))


def meta_rows(tgt, lw, coef):
    m = np.zeros((len(tgt), 4), np.float32)
    m[:, 0] = np.asarray(tgt, np.int32).view(np.float32); m[:, 1] = lw; m[:, 2] = coef
    return m


def vp_call(dev, dt, stages, det=0, idx=None, label=None, weight=None, position=None, stats=None, npos=None, task_w=0.0, KB=0, KBmax=1,
            own=None, EwAll=None, metaAll=None, W=1, D=8, EwC=None, metaC=None, nlive=None, pre=None, logits=None, ldl=0, Vloc=0, col0=0,
            lmax=None, gmax=None, sums=None, cap=1, rank=0, loss=None, rows=0, rows_finish=0):
    return dev.L.rsys_op_vp_ce(dt, stages, det, idx, label, weight, position, stats, npos, f(task_w), KB, KBmax, own, EwAll, metaAll, W, D, EwC,
                               metaC, nlive, pre, logits, ldl, Vloc, col0, lmax, gmax, sums, cap, rank, loss, rows, rows_finish)


def ss_call(dev, dt, stages, det=0, length=0, n_s=0, n_tot=0, col0=0, seed=0, stream=0, cols=None, bitmap=None, tlist=None, tcount=None,
            metaC=None, nlive=None, pre=None, rank=0, cap_rows=0, rows=0, rows_finish=0, EwC=None, Floc=None, D=0, logits=None, ldl=0,
            lmax=None, lsum=None, tl=None, gmax=None, loss=None, dt_=None, gE=None, dEwC=None, ridx=None, rbase=0, rld=0, rn=0, rtable=0,
            gsrc=None, gdst=None, asrc=None, adst=None):
    return dev.L.rsys_op_ss(dt, stages, det, length, n_s, n_tot, col0, seed, stream, cols, bitmap, tlist, tcount, metaC, nlive, pre, rank,
                            cap_rows, rows, rows_finish, EwC, Floc, D, logits, ldl, lmax, lsum, tl, gmax, loss, dt_, gE, dEwC, ridx, rbase, rld,
                            rn, rtable, gsrc, gdst, asrc, adst)


def rows_call(dev, stages, skey=None, sidx=None, N=0, V=0, slot=None, uniq=None, tok2u=None, plan=None, bound=None, nb=0, off=None,
              table=None, ld=0, table_rows=0, ids=None, sub=0, packed=None, n=0, D=0, count=None, mid=None, uid=None, tm=None, Ntok=0,
              Frem=None, frem_rows=0, x0=None, uid_t=None, tm_t=None):
    return dev.L.rsys_op_shard_rows(stages, skey, sidx, N, V, slot, uniq, tok2u, plan, bound, nb, off, table, ld, table_rows, ids, sub, packed,
                                    n, D, count, mid, uid, tm, Ntok, Frem, frem_rows, x0, uid_t, tm_t)


# ============================================================================================ vp_meta / vp_compact
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("W,KB,KBmax,D", [(1, 1, 3, 8), (3, 5, 8, 136), (47, 64, 70, 512)])
def test_vp_meta_and_compact(dev, dt, W, KB, KBmax, D):
    rng = np.random.default_rng(W + D)
    N = KB + 9
    for variant in ("random", "full", "none"):
        counts = {"random": rng.integers(0, KB + 1, W), "full": np.full(W, KB), "none": np.zeros(W, int)}[variant]
        if variant == "random" and W > 2:
            counts[0] = KB; counts[1] = 0
        metaAll = np.zeros((W, KBmax * 4 + 4), np.float32)
        want_rows = []
        for q in range(W):
            idx = rng.permutation(N)[:KB].astype(np.int32)
            label = rng.uniform(0.5, 1.5, N).astype(np.float32); weight = rng.uniform(0.2, 2.0, N).astype(np.float32)
            weight[idx[1::3]] = 0.0
            pos = rng.integers(0, 100000, N).astype(np.int32)
            small = q % 3 == 1 or (W == 1 and variant == "full")                 # stats[0] < 1e-8: the divisor is 1e-8
            stats0 = np.float32(3e-9 if small else rng.uniform(1.0, 5.0)); task_w = np.float32(0.3)
            down = dev.put(np.full(KBmax * 4 + 1, SENT, np.float32))
            _ok(vp_call(dev, dt, 1, idx=dev.puti(idx), label=dev.put(label), weight=dev.put(weight), position=dev.puti(pos),
                        stats=dev.put(np.array([stats0, 0], np.float32)), npos=dev.puti([counts[q]]), task_w=task_w, KB=KB, KBmax=KBmax, own=down))
            own = dev.get(down, (KBmax * 4 + 1,))
            lw = label[idx] * weight[idx]                                     # fp32 products and quotient, as the kernel forms them
            want = meta_rows(pos[idx], lw, task_w * lw / np.maximum(stats0, np.float32(1e-8)))
            assert np.array_equal(own[:KB * 4].view(np.uint32), want.ravel().view(np.uint32)), (variant, q)
            assert np.all(own[KB * 4:KBmax * 4] == 0) and own[KBmax * 4:].view(np.int32)[0] == counts[q]
            metaAll[q, :KBmax * 4 + 1] = own
            want_rows.append(want)
        EwAll = storage(rng.standard_normal((W, KBmax, D)), dt)
        cap = W * KBmax
        dE = dev.put(np.full((cap, D), SENT, np.float32), dt); dM = dev.put(np.full((cap, 4), SENT, np.float32))
        dn = dev.puti([ISENT]); dp = dev.puti(np.full(W + 1, ISENT))
        _ok(vp_call(dev, dt, 2, EwAll=dev.put(EwAll, dt), metaAll=dev.put(metaAll), W=W, KBmax=KBmax, D=D, EwC=dE, metaC=dM, nlive=dn, pre=dp))
        nlive, pre, src = sn.vp_compact(counts, KB)
        assert dev.geti(dn, (1,))[0] == nlive and np.array_equal(dev.geti(dp, (W + 1,)), pre)
        E = dev.get(dE, (cap, D), dt); M = dev.get(dM, (cap, 4))
        for row, (q, i) in enumerate(src):
            assert np.array_equal(E[row], EwAll[q, i]) and np.array_equal(M[row].view(np.uint32), want_rows[q][i].view(np.uint32)), (row, q, i)
        z = min((nlive + 255) // 256 * 256, cap)
        assert np.all(M[nlive:z] == 0) and np.all(M[z:] == SENT) and np.all(E[nlive:] == SENT), variant


# ============================================================================================ the vp chain
VP_CASES = [  # (column split over the ranks, live rows per rank, KBmax): cap = W KBmax
    ((1,), (1,), 300),
    ((7, 8, 9), (128, 0, 127), 128),             # 255 live rows; a rank with no rows and one with KBmax
    ((0, 1025, 7), (128, 128, 0), 128),          # 256; an empty range in front; one column past a whole fp32 sweep
    ((2049, 0, 1023), (90, 77, 90), 90),         # 257 > cap rounded: npad = cap = 270; one column past a whole bf16 sweep
    ((4100, 2051), (300, 0), 300),               # 300; four fp32 / two bf16 sweeps and a ragged tail
]


def _vp_rows(rng, n, split, dt):
    V = sum(split)
    col0 = np.concatenate([[0], np.cumsum(split)])
    X = rng.standard_normal((n, V)) * 3.0
    edges = sorted({int(c) for q, v in enumerate(split) if v for c in (col0[q], col0[q] + v - 1)})   # first / last column of every range:
    tgt = rng.integers(0, V, n)                                                                       # for its neighbour, col0 - 1 / col0 + Vloc
    tgt[:len(edges)] = edges[:n]
    if n > 2 * len(edges):
        tgt[-len(edges):] = edges
    for row in range(n):
        X[row] += (0.0, 80.0, -80.0, 1e4, -1e4, 0.0)[row % 6]
        if row % 6 == 5:
            X[row, tgt[row]] = 40.0                                       # peaked: the target holds nearly all the mass
    lw = (rng.uniform(0.5, 1.5, n).astype(np.float32) * rng.uniform(0.2, 2.0, n).astype(np.float32))
    lw[1::4] = 0.0                                                        # label weight 0: no loss term, a zero gradient row
    div = np.where(np.arange(n) % 7 == 3, np.float32(1e-8), np.float32(2.5))   # stats[0] < 1e-8: the divisor is 1e-8
    coef = (np.float32(0.3) * lw / div).astype(np.float32)
    return storage(X, dt), tgt, lw, coef, col0


def _sweep_len(Vloc, dt):
    E = 8 if dt == BF16 else 4
    return E * -(-(-(-Vloc // E)) // 256)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("case", range(len(VP_CASES)))
def test_vp_chain(dev, dt, det, case):
    split, counts, KBmax = VP_CASES[case]
    W = len(split); cap = W * KBmax
    rng = np.random.default_rng(case + 10 * dt)
    nlive, pre, src = sn.vp_compact(counts, KBmax)
    npad = min(cap, (nlive + 255) // 256 * 256)
    X, tgt, lw, coef, col0 = _vp_rows(rng, nlive, split, dt)
    # compact: the packed meta, nlive and pre come from the kernel (8-column payload rows)
    metaAll = np.zeros((W, KBmax * 4 + 4), np.float32)
    mrows = meta_rows(tgt, lw, coef)
    for q in range(W):
        metaAll[q, :counts[q] * 4] = mrows[pre[q]:pre[q + 1]].ravel()
        metaAll[q, KBmax * 4:KBmax * 4 + 1] = np.array([counts[q]], np.int32).view(np.float32)
    dM = dev.put(np.full((cap, 4), SENT, np.float32)); dn = dev.puti([ISENT]); dp = dev.puti(np.full(W + 1, ISENT))
    _ok(vp_call(dev, dt, 2, EwAll=dev.put(np.zeros((W, KBmax, 8)), dt), metaAll=dev.put(metaAll), W=W, KBmax=KBmax, D=8,
                EwC=dev.put(np.zeros((cap, 8)), dt), metaC=dM, nlive=dn, pre=dp))
    assert dev.geti(dn, (1,))[0] == nlive and np.array_equal(dev.geti(dp, (W + 1,)), pre)
    ref = sn.vp_ce([X[:, col0[q]:col0[q + 1]].astype(np.float64) for q in range(W)], col0[:-1], tgt, lw.astype(np.float64),
                   coef.astype(np.float64), pre)

    def run():
        """the whole chain; returns per rank (lmax, sums, tl), the reduced arrays, per rank (loss, dlogits block)"""
        bufs = []; st = []
        for q in range(W):
            Vloc = split[q]; ldl = (Vloc + 7) // 8 * 8
            L = np.full((cap, ldl), SENT, np.float64)
            L[:npad] = np.nan                                   # NaN in the padding columns and in rows [nlive, npad)
            L[:nlive, :Vloc] = X[:, col0[q]:col0[q + 1]]
            dL = dev.put(L, dt) if ldl else None
            dlm = dev.put(np.full(cap, SENT, np.float32)); dsm = dev.put(np.full(2 * cap, SENT, np.float32))
            _ok(vp_call(dev, dt, 4, logits=dL, ldl=ldl, Vloc=Vloc, col0=int(col0[q]), metaC=dM, nlive=dn, lmax=dlm, sums=dsm, cap=cap, rows=nlive))
            lm = dev.get(dlm, (cap,)); sm = dev.get(dsm, (2, cap))
            assert np.all(lm[nlive:] == SENT) and np.all(sm[:, nlive:] == SENT)      # the grid is nlive rows: nothing behind them
            bufs.append((dL, dlm, dsm, ldl)); st.append((lm[:nlive].copy(), sm[0, :nlive].copy(), sm[1, :nlive].copy()))
        gmax = np.max([s[0] for s in st], 0)                    # max all-reduce: exact
        reb = []
        for q in range(W):
            dL, dlm, dsm, ldl = bufs[q]
            dg = dev.put(np.concatenate([gmax, np.full(cap - nlive, SENT, np.float32)]))
            _ok(vp_call(dev, dt, 8, metaC=dM, nlive=dn, logits=dL, ldl=ldl, Vloc=split[q], lmax=dlm, gmax=dg, sums=dsm, cap=cap, rows=nlive))
            reb.append(dev.get(dsm, (2, cap))[0, :nlive].copy())
        S = np.zeros(nlive, np.float32); T = np.zeros(nlive, np.float32)
        for q in range(W):                                      # sum all-reduces: fp32, rank order
            S = S + reb[q]; T = T + st[q][2]
        out = []
        for q in range(W):
            dL, dlm, dsm, ldl = bufs[q]
            sums = np.full((2, cap), SENT, np.float32); sums[0, :nlive] = S; sums[1, :nlive] = T
            dg = dev.put(np.concatenate([gmax, np.full(cap - nlive, SENT, np.float32)]))
            dloss = dev.put(np.array([1.5], np.float32))        # the loss is added to
            _ok(vp_call(dev, dt, 16, det=det, logits=dL, ldl=ldl, Vloc=split[q], col0=int(col0[q]), metaC=dM, gmax=dg, sums=dev.put(sums),
                        cap=cap, nlive=dn, pre=dp, rank=q, loss=dloss, rows_finish=npad))
            out.append((float(dev.get(dloss, (1,))[0]) - 1.5, dev.get(dL, (cap, ldl), dt) if ldl else np.zeros((cap, 0), np.float32)))
        return st, gmax, reb, S, out

    st, gmax, reb, S, out = run()
    R = X.astype(np.float64).max(1) - X.astype(np.float64).min(1)
    e_S = np.zeros(nlive)
    for q in range(W):
        lm, sm, tlq = st[q]
        if split[q] == 0:                                        # an empty range: the neutral elements
            assert np.all(lm == NEG) and np.all(sm == 0) and np.all(tlq == 0) and np.all(reb[q] == 0)
            continue
        assert np.array_equal(lm, ref["lmax"][q].astype(np.float32))              # a maximum of stored values: exact
        assert np.array_equal(tlq, ref["tl"][q].astype(np.float32))               # a copy (0 where the target is a neighbour's)
        c_loc = 7 * _sweep_len(split[q], dt) + 6 * R + 24
        note("vp_stats", np.abs(sm - ref["sums"][q]), c_loc * U * ref["sums"][q])
        c_reb = c_loc + 4 + 2 * (ref["gmax"] - ref["lmax"][q])
        note("vp_rebase", np.abs(reb[q] - ref["reb"][q]), c_reb * U * ref["reb"][q])
        e_S = np.maximum(e_S, c_reb * U)
    assert np.array_equal(gmax, ref["gmax"].astype(np.float32))
    Sref = ref["reb"].sum(0)
    e_S = e_S + W * U
    note("vp sum", np.abs(S - Sref), e_S * Sref)
    lse = ref["lse"]; tl = ref["tl"].sum(0)
    e_lse = e_S + U * (2 * np.abs(np.log(Sref)) + 2 * np.abs(lse))
    term_b = e_lse * np.abs(lw) + 2 * U * np.abs(ref["term"])
    for q in range(W):
        loss, dX = out[q]
        own = slice(pre[q], pre[q + 1])
        # only this rank's rows: the other rows' terms are far outside the bound, so a term from a foreign row fails here
        note("vp_finish loss", abs(loss - ref["loss"][q]),
             term_b[own].sum() + (counts[q] + 1) * U * (np.abs(ref["term"][own]).sum() + 1.5) + 1e-300)
        Vloc = split[q]
        Xq = X[:, col0[q]:col0[q + 1]].astype(np.float64)
        d = ref["dl"][q]
        p = np.exp(Xq - lse[:, None])
        bound = np.abs(coef)[:, None] * (p * (e_lse[:, None] + 2 * U * np.abs(Xq - lse[:, None]) + 3 * U) + 2.0 ** -125) + 3 * U * np.abs(d)
        if dt == BF16:
            bound = bound + bf16_ulp(d)
        note("vp_finish dlogits", np.abs(dX[:nlive, :Vloc] - d), bound)
        assert np.all(dX[:nlive, :Vloc][lw == 0] == 0)                             # label weight 0: an exactly zero row
        assert np.all(dX[:nlive, Vloc:] == 0)                                      # zeros in [Vloc, ldl), whatever the GEMM left there
        assert np.all(dX[nlive:npad] == 0)                                         # rows [nlive, npad): zeros
        assert np.all(dX[npad:] == SENT)                                           # rows >= npad: untouched
    assert abs(sum(o[0] for o in out) - ref["term"].sum()) <= term_b.sum() + (nlive + W) * U * (np.abs(ref["term"]).sum() + 1.5 * W)
    if det:
        again = run()[4]
        assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(out, again))


# ============================================================================================ ss_sample
SAMPLE_SHAPES = [(1, 1), (5, 5), (7, 3), (10, 3), (1000, 256), (200003, 4096)]


def _sample(dev, length, n_s, seed, stream):
    dc = dev.puti(np.full(n_s, ISENT))
    _ok(ss_call(dev, F32, 1, length=length, n_s=n_s, n_tot=n_s, seed=seed, stream=stream, cols=dc))
    return dev.geti(dc, (n_s,))


@pytest.mark.parametrize("length,n_s", SAMPLE_SHAPES)
def test_ss_sample(dev, length, n_s):
    seed, stream = 0x9E3779B97F4A7C15, 2 * 1000 + 1
    cols = _sample(dev, length, n_s, seed, stream)
    assert np.array_equal(cols, sn.ss_sample(length, n_s, seed, stream))          # the Philox restatement, entry by entry
    lo = sn.stratum_lo(np.arange(n_s + 1), length, n_s)
    assert np.all(cols >= lo[:-1]) and np.all(cols < lo[1:])                      # one class inside each stratum
    for s2, t2 in ((seed, stream + 1), (seed ^ (1 << 40), stream), (0x1234567, 0xFFFFFFFF)):
        other = _sample(dev, length, n_s, s2, t2)
        assert np.array_equal(other, sn.ss_sample(length, n_s, s2, t2))
        if n_s >= 256:
            assert 0 < (other != cols).mean()                                     # the columns change with the stream and with the seed
            assert (other != cols).mean() > 0.5
    dc = dev.puti(np.full(length + 1, ISENT))
    rc = ss_call(dev, F32, 1, length=length, n_s=length + 1, n_tot=length + 1, seed=seed, stream=stream, cols=dc)
    assert rc == -1 and "samples" in _lib().last_error()                          # RSYS_ERR_ARG, nothing launched
    assert np.all(dev.geti(dc, (length + 1,)) == ISENT)


# ============================================================================================ ss_targets / ss_drop_hits
@pytest.mark.parametrize("length", [1, 31, 32, 33, 32768, 32769, 70001])
@pytest.mark.parametrize("nlive", [1, 300])
def test_ss_targets_and_drop_hits(dev, length, nlive):
    rng = np.random.default_rng(length + nlive)
    col0, cap_rows = 1000, nlive + 77
    loc = rng.integers(0, length, cap_rows)
    loc[:nlive][rng.random(nlive) < 0.3] = length - 1                             # duplicates, the last class
    if nlive > 4:
        loc[0] = 0; loc[1] = -1; loc[2] = length; loc[3] = -col0; loc[4] = loc[5]  # the first class; a neighbour's on either side; id 0
    # rows [nlive, cap_rows) hold stale meta that names local classes: they must not be marked
    want = np.unique(loc[:nlive][(loc[:nlive] >= 0) & (loc[:nlive] < length)])
    dM = dev.put(meta_rows(loc + col0, np.ones(cap_rows), np.ones(cap_rows)))
    words = (length + 31) // 32
    dB = dev.puti(np.full(words, -1)); dT = dev.puti(np.full(nlive + 8, ISENT)); dC = dev.puti([ISENT])
    args = dict(length=length, col0=col0, metaC=dM, nlive=dev.puti([nlive]), cap_rows=cap_rows, bitmap=dB, tlist=dT, tcount=dC)
    _ok(ss_call(dev, F32, 2, **args))
    n_t = dev.geti(dC, (1,))[0]
    tl = dev.geti(dT, (nlive + 8,))
    assert n_t == len(want) and np.array_equal(tl[:n_t], want) and np.all(tl[n_t:] == ISENT)
    bits = np.unpackbits(dev.geti(dB, (words,)).view(np.uint8), bitorder="little")
    assert np.array_equal(np.nonzero(bits)[0], want)
    n_s = min(length, 300)
    cols = sn.ss_sample(length, n_s, 7, 3)
    take = rng.permutation(n_s)[:max(1, n_s // 3)]                               # a third of the samples land on a marked class
    cols[take] = rng.choice(want, len(take)) if len(want) else cols[take]
    dcols = dev.puti(cols)
    _ok(ss_call(dev, F32, 4, length=length, n_s=n_s, n_tot=n_s, cols=dcols, bitmap=dB))
    hit = np.isin(cols, want)
    assert hit.any() or not len(want)
    assert np.array_equal(dev.geti(dcols, (n_s,)), np.where(hit, -1, cols))
    rc = ss_call(dev, F32, 4, length=length, n_s=n_s, n_tot=n_s, cols=dev.puti(np.full(n_s, length)), bitmap=dB)
    assert rc == -1                                                               # a column outside the bitmap is refused, not read


# ============================================================================================ plain row copies and rows by id
@pytest.mark.parametrize("D", [8, 136, 2048])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_rows_plain_and_by_id(dev, D, n):
    rng = np.random.default_rng(D + n)
    ld, base, trows = D + 8, 3, n + 9
    idx = rng.permutation(trows - base)[:n].astype(np.int32)
    idx[::4] = -1 if n > 1 else idx[::4]
    for dt in DTYPES:
        tab = storage(rng.standard_normal((trows, ld)), dt)
        dd = dev.put(np.full((n + 2, D), SENT, np.float32), dt)
        _ok(ss_call(dev, dt, 8, D=D, ridx=dev.puti(idx), rbase=base, rld=ld, rn=n, rtable=trows, gsrc=dev.put(tab, dt), gdst=dd))
        got = dev.get(dd, (n + 2, D), dt)
        want = np.where(idx[:, None] >= 0, tab[base + np.maximum(idx, 0), :D], 0.0)
        assert np.array_equal(got[:n], want) and np.all(got[n:] == SENT)
    tab = rng.standard_normal((trows, ld)).astype(np.float32); src = rng.standard_normal((n, D)).astype(np.float32)
    dtab = dev.put(tab)
    _ok(ss_call(dev, F32, 512, D=D, ridx=dev.puti(idx), rbase=base, rld=ld, rn=n, rtable=trows, asrc=dev.put(src), adst=dtab))
    want = tab.copy()
    for j in range(n):
        if idx[j] >= 0:
            want[base + idx[j], :D] += src[j]
    assert np.array_equal(dev.get(dtab, (trows, ld)), want)
    rc = ss_call(dev, F32, 512, D=D, ridx=dev.puti(np.full(n, trows)), rbase=base, rld=ld, rn=n, rtable=trows, asrc=dev.put(src), adst=dtab)
    assert rc == -1
    # rows by id: ids are table rows + sub
    sub = 40
    ids = (rng.permutation(trows)[:n] + sub).astype(np.int32)
    dpk = dev.put(np.full((n + 2, D), SENT, np.float32))
    _ok(rows_call(dev, 4, table=dev.put(tab), ld=ld, table_rows=trows, ids=dev.puti(ids), sub=sub, packed=dpk, n=n, D=D))
    got = dev.get(dpk, (n + 2, D))
    assert np.array_equal(got[:n], tab[ids - sub, :D]) and np.all(got[n:] == SENT)
    dpk = dev.put(np.full((n + 2, D), SENT, np.float32))                         # no rows: no launch, no error, nothing written
    _ok(rows_call(dev, 4, table=dev.put(tab), ld=ld, table_rows=trows, ids=dev.puti(ids), sub=sub, packed=dpk, n=0, D=D))
    assert np.all(dev.get(dpk, (n + 2, D)) == SENT)
    dtab = dev.put(tab)
    _ok(rows_call(dev, 8, table=dtab, ld=ld, table_rows=trows, ids=dev.puti(ids), sub=sub, packed=dev.put(src), n=n, D=D))
    want = tab.copy(); want[ids - sub, :D] += src
    assert np.array_equal(dev.get(dtab, (trows, ld)), want)
    for count in (n - 1, n, n + 5):                                              # *count below, equal to and above the capacity
        dtab = dev.put(tab)
        _ok(rows_call(dev, 16, table=dtab, ld=ld, table_rows=trows, ids=dev.puti(ids - sub), packed=dev.put(src), n=n, D=D,
                      count=dev.puti([count])))
        k = min(count, n)
        want = tab.copy(); want[(ids - sub)[:k], :D] += src[:k]
        assert np.array_equal(dev.get(dtab, (trows, ld)), want), count


# ============================================================================================ exchange plan
@pytest.mark.parametrize("N", [1, 63, 64, 1023, 1024, 1025, 5000])
@pytest.mark.parametrize("keys", ["masked", "none_masked", "one_id", "distinct", "zipf"])
def test_exchange_plan(dev, N, keys):
    rng = np.random.default_rng(N)
    V = 7000
    ids = {"masked": np.full(N, -1), "none_masked": rng.integers(0, V, N), "one_id": np.full(N, 4242),
           "distinct": rng.permutation(V)[:N], "zipf": (rng.zipf(1.3, N) - 1) % V}[keys]
    if keys == "zipf":
        ids[::5] = -1
    if keys == "none_masked" and N > 1:
        ids[0] = V - 1; ids[1] = 0
    key = np.where(ids < 0, V, ids)
    sidx = np.argsort(key, kind="stable").astype(np.int32); skey = key[sidx].astype(np.int32)
    ds, du, dtk, dpl = dev.puti(np.full(N, ISENT)), dev.puti(np.full(N + 1, ISENT)), dev.puti(np.full(N, ISENT)), dev.puti([ISENT, ISENT])
    _ok(rows_call(dev, 1, skey=dev.puti(skey), sidx=dev.puti(sidx), N=N, V=V, slot=ds, uniq=du, tok2u=dtk, plan=dpl))
    slot, uniq, tok2u, (Uq, uV) = sn.plan_unique(skey, sidx, V)
    assert list(dev.geti(dpl, (2,))) == [Uq, uV]
    got_u = dev.geti(du, (N + 1,))
    assert np.array_equal(got_u[:Uq], uniq) and np.all(got_u[Uq:] == ISENT)
    assert np.array_equal(dev.geti(ds, (N,)), slot) and np.array_equal(dev.geti(dtk, (N,)), tok2u)
    for nb in (2, 4, 48):
        cuts = np.sort(rng.integers(0, V + 1, nb - 2))
        if nb > 4:
            cuts[3] = cuts[2]; cuts[-1] = V + 1; cuts[0] = 0                      # empty owner ranges, in front and behind too
            cuts = np.sort(cuts)
        bound = np.concatenate([[0], cuts, [V + 1]]).astype(np.int32)
        doff = dev.puti(np.full(nb + 3, ISENT))
        _ok(rows_call(dev, 2, uniq=du, plan=dpl, bound=dev.puti(bound), nb=nb, off=doff))
        off = dev.geti(doff, (nb + 3,))
        assert np.array_equal(off[:nb], sn.plan_offsets(uniq, bound)) and np.all(off[nb:] == ISENT) and off[nb - 1] == Uq
    D = 136 if N < 2000 else 8
    Frem = rng.standard_normal((Uq, D)).astype(np.float32)
    uid = rng.integers(0, 1 << 19, N).astype(np.int32); tm = rng.integers(0, 4096, N).astype(np.int32)
    m_mid = ids.copy(); m_mid[rng.random(N) < 0.2] = -1                           # watch-masked tokens: they read the mask row's slot uV
    dx, dut, dtt = dev.put(np.full((2 * N, D), SENT, np.float32)), dev.puti(np.full(2 * N, ISENT)), dev.puti(np.full(2 * N, ISENT))
    _ok(rows_call(dev, 32, mid=dev.puti(m_mid), uid=dev.puti(uid), tm=dev.puti(tm), Ntok=N, Frem=dev.put(Frem), frem_rows=Uq, tok2u=dtk,
                  plan=dpl, D=D, x0=dx, uid_t=dut, tm_t=dtt))
    x0 = dev.get(dx, (N, 2, D))
    assert np.array_equal(x0[:, 0], Frem[np.where(m_mid == -1, uV, tok2u)]) and np.all(x0[:, 1] == SENT)
    assert np.array_equal(dev.geti(dut, (N, 2)), np.stack([uid, uid], 1)) and np.array_equal(dev.geti(dtt, (N, 2)), np.stack([tm, tm], 1))


# ============================================================================================ ss_target_logit
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [64, 136, 520, 2048])
def test_ss_target_logit(dev, dt, D):
    rng = np.random.default_rng(D)
    length, col0, nlive, rows = 11, 500, 9, 12
    loc = rng.integers(0, length, rows)
    loc[0] = 0; loc[1] = length - 1; loc[2] = -1; loc[3] = length; loc[4] = -col0     # not local: a neighbour's, or far away
    Ew = storage(rng.standard_normal((rows, D)), dt); Fl = storage(rng.standard_normal((length, D)), dt)
    dtl = dev.put(np.full(rows, SENT, np.float32))
    _ok(ss_call(dev, dt, 16, length=length, col0=col0, metaC=dev.put(meta_rows(loc + col0, np.ones(rows), np.ones(rows))),
                nlive=dev.puti([nlive]), rows=rows, EwC=dev.put(Ew, dt), Floc=dev.put(Fl, dt), D=D, tl=dtl))
    tl = dev.get(dtl, (rows,))
    local = (loc >= 0) & (loc < length)
    prod = Ew.astype(np.float64) * Fl[np.clip(loc, 0, length - 1)].astype(np.float64)
    want = np.where(local, prod.sum(1), 0.0)
    note("ss_target_logit", np.abs(tl[:nlive] - want[:nlive]), (2 * -(-D // 64) + 6) * U * np.abs(prod).sum(1)[:nlive] + 1e-300)
    assert np.all(tl[:nlive][~local[:nlive]] == 0) and np.all(tl[nlive:] == SENT)


# ============================================================================================ the ss chain
SS_CASES = [  # ((len, n_s) per rank, live rows)
    ([(1000, 256)], 300),                        # 300 rows with distinct targets: n_tot > 256, the sweep runs twice
    ([(37, 8), (0, 0)], 1),
    ([(12, 12), (37, 8), (1000, 256)], 130),
]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("case", range(len(SS_CASES)))
def test_ss_chain(dev, dt, det, case):
    shapes, nlive = SS_CASES[case]
    W = len(shapes)
    rng = np.random.default_rng(case + 10 * dt)
    lens = [s[0] for s in shapes]
    col0 = np.concatenate([[0], np.cumsum(lens)]) + 50
    Vtot = sum(lens)
    cap = nlive + 300
    npad = min(cap, (nlive + 255) // 256 * 256)
    pre = np.linspace(0, nlive, W + 1).astype(np.int32)
    tgt = 50 + rng.integers(0, Vtot, nlive)
    if case == 0:
        tgt = 50 + rng.permutation(1000)[:nlive]                                   # 300 distinct in-batch targets
    if case == 2:
        tgt[0:6] = col0[0] + rng.integers(0, 12, 6); tgt[6:16] = col0[1] + rng.permutation(37)[:10]   # rows for the two small ranks too
    lw = rng.uniform(0.2, 2.0, nlive).astype(np.float32); lw[1::4] = 0.0
    coef = (np.float32(0.3) * lw / np.where(np.arange(nlive) % 7 == 3, np.float32(1e-8), np.float32(2.5))).astype(np.float32)
    shift = np.array([(0.0, 80.0, -80.0, 1e4, -1e4)[r % 5] for r in range(nlive)])
    tlv = storage(rng.standard_normal(nlive) * 3.0 + shift + np.where(np.arange(nlive) % 6 == 5, 40.0, 0.0), F32)   # every 6th row peaked
    ranks = []; hit_slots = []; drop_slots = []; sampled_hits = 0
    for q, (length, n_s) in enumerate(shapes):
        if n_s == 0:
            ranks.append(dict(X=np.zeros((nlive, 0)), cols=np.zeros(0, np.int32), n_s=0, len=length, col0=col0[q], tgt=tgt)); continue
        cols = sn.ss_sample(length, n_s, 99 + q, 5)
        T = np.zeros(0, np.int32)
        rows_q = np.nonzero((tgt >= col0[q]) & (tgt < col0[q] + length))[0]
        if n_s < length:
            if len(rows_q):
                tgt[rows_q[0]] = col0[q] + cols[0]                                  # sample 0 is an in-batch target: dropped
            loc = tgt - col0[q]
            T = np.unique(loc[rows_q]).astype(np.int32)
            # an accidental hit among the SAMPLED slots: one row's class is left out of the list and slot 1 is given that class
            cand = [int(r) for r in rows_q[1:] if (loc == loc[r]).sum() == 1 and loc[r] != cols[0]]
            if cand:
                cls = loc[cand[0]]
                cols[1] = cls; T = T[T != cls]; hit_slots.append((q, cand[0], 1)); sampled_hits += 1
            drop = np.isin(cols, T)
            cols = np.where(drop, -1, cols).astype(np.int32)
            drop_slots += [(q, int(c)) for c in np.nonzero(drop)[0]]
            hit_slots += [(q, int(r), n_s + int(np.searchsorted(T, loc[r]))) for r in rows_q if loc[r] in T]   # the row's own list entry
        else:
            loc = tgt - col0[q]
            hit_slots += [(q, int(r), int(loc[r])) for r in rows_q]                 # every class sampled: slot = class
        cl = np.concatenate([cols, T]).astype(np.int32)
        X = rng.standard_normal((nlive, len(cl))) * 3.0 + shift[:, None]
        for (qq, r, c) in hit_slots:
            if qq == q:
                assert cl[c] == tgt[r] - col0[q]
                X[r, c] = shift[r] + 50.0                                           # a hit is skipped: were it counted, it would dominate
        X = storage(X, dt).astype(np.float64)
        ranks.append(dict(X=X, cols=cl, n_s=n_s, len=length, col0=col0[q], tgt=tgt))
    assert drop_slots and hit_slots and (sampled_hits or nlive == 1)
    if case == 0:
        assert len(ranks[0]["cols"]) > 256
    mrows = meta_rows(tgt, lw, coef)
    meta = np.full((cap, 4), SENT, np.float32); meta[:nlive] = mrows
    meta[nlive:, 0] = np.asarray(tgt[0], np.int32).view(np.float32)                # stale meta behind the live rows
    dM = dev.put(meta); dn = dev.puti([nlive]); dp = dev.puti(pre)
    ref = sn.ss_chain(ranks, tlv.astype(np.float64), lw.astype(np.float64), coef.astype(np.float64), pre)

    def run():
        bufs = []; st = []
        for q, r in enumerate(ranks):
            n_tot = len(r["cols"]); ldl = (max(n_tot, 8) + 7) // 8 * 8
            L = np.full((cap, ldl), SENT, np.float64)
            L[:npad] = np.nan
            L[:nlive, :n_tot] = np.where(r["cols"][None, :] >= 0, r["X"], np.nan)   # a dropped entry's logit is never read
            dL = dev.put(L, dt); dc = dev.puti(r["cols"]) if n_tot else dev.puti([ISENT])
            dlm = dev.put(np.full(cap, SENT, np.float32)); dls = dev.put(np.full(cap, SENT, np.float32))
            dtl = dev.put(np.concatenate([tlv, np.full(cap - nlive, SENT, np.float32)]))   # (the tl sum: one owner, the rest zeros: exact)
            dg = dev.put(np.full(cap, SENT, np.float32))
            kw = dict(length=r["len"], n_s=r["n_s"], n_tot=n_tot, col0=int(r["col0"]), cols=dc, metaC=dM, nlive=dn, logits=dL, ldl=ldl,
                      lmax=dlm, lsum=dls, tl=dtl, gmax=dg, rows=nlive)
            _ok(ss_call(dev, dt, 32 | 64, **kw))
            lm = dev.get(dlm, (cap,)); ls = dev.get(dls, (cap,)); g = dev.get(dg, (cap,))
            assert np.all(lm[nlive:] == SENT) and np.all(ls[nlive:] == SENT) and np.all(g[nlive:] == SENT)
            assert np.array_equal(g[:nlive], np.maximum(lm[:nlive], tlv))
            bufs.append((kw, dL, dls, ldl)); st.append((lm[:nlive].copy(), ls[:nlive].copy(), g[:nlive].copy()))
        gmax = np.max([s[2] for s in st], 0)
        S = np.zeros(nlive, np.float32); reb = []
        for q in range(W):
            kw = dict(bufs[q][0]); kw["gmax"] = dev.put(np.concatenate([gmax, np.full(cap - nlive, SENT, np.float32)]))
            _ok(ss_call(dev, dt, 128, **kw))
            reb.append(dev.get(bufs[q][2], (cap,))[:nlive].copy())
            S = S + reb[q]
        out = []
        for q in range(W):
            kw = dict(bufs[q][0]); ldl = bufs[q][3]
            kw["gmax"] = dev.put(np.concatenate([gmax, np.full(cap - nlive, SENT, np.float32)]))
            kw["lsum"] = dev.put(np.concatenate([S, np.full(cap - nlive, SENT, np.float32)]))
            dloss = dev.put(np.array([1.5], np.float32)); ddt = dev.put(np.full(cap, SENT, np.float32))
            _ok(ss_call(dev, dt, 256, det=det, pre=dp, rank=q, loss=dloss, dt_=ddt, rows_finish=npad, **kw))
            out.append((float(dev.get(dloss, (1,))[0]) - 1.5, dev.get(bufs[q][1], (cap, ldl), dt), dev.get(ddt, (cap,))))
        return st, gmax, reb, S, out

    st, gmax, reb, S, out = run()
    e_S = np.zeros(nlive)
    for q, r in enumerate(ranks):
        lm, ls, _ = st[q]
        n_tot = len(r["cols"])
        if n_tot == 0:
            assert np.all(lm == NEG) and np.all(ls == 0) and np.all(reb[q] == 0)
            continue
        a = ref["act"][q]
        w = sn.ss_weights(r["len"], r["n_s"], n_tot)
        y = r["X"] + np.log(w)[None, :]
        dy = np.where(a, U * (4 * np.log(w)[None, :] + np.abs(y)), 0.0).max(1)
        has = a.any(1)
        with np.errstate(invalid="ignore"):
            R = np.where(has, np.where(a, y, -np.inf).max(1) - np.where(a, y, np.inf).min(1), 0.0)
        assert np.all(lm[~has] == NEG) and np.all(ls[~has] == 0)
        note("ss_stats lmax", np.abs(lm[has] - ref["lmax"][q][has]), dy[has] + 1e-300)
        c_loc = (7 * -(-n_tot // 256) + 6 * R + 24) * U + 2 * dy
        note("ss_stats lsum", np.abs(ls - ref["lsum"][q]), c_loc * ref["lsum"][q] + 1e-300)
        c_reb = c_loc + (4 + 2 * np.abs(ref["gmax"] - ref["lmax"][q])) * U + dy       # (+ dy: the kernel's gmax is its own lmax's)
        note("ss_rebase", np.abs(reb[q] - ref["sneg_q"][q]) * has, c_reb * ref["sneg_q"][q] + 1e-300)
        e_S = np.maximum(e_S, np.where(has, c_reb, 0.0))
    e_S = e_S + W * U
    note("ss sum", np.abs(S - ref["sneg"]), e_S * ref["sneg"] + 1e-300)
    tl64 = tlv.astype(np.float64); lse = ref["lse"]
    Sig = np.exp(tl64 - ref["gmax"]) + ref["sneg"]
    e_lse = e_S + (4 + 2 * np.abs(tl64 - ref["gmax"])) * U + U * (2 * np.abs(np.log(Sig)) + 2 * np.abs(lse))
    term_b = e_lse * np.abs(lw) + 2 * U * np.abs(ref["term"])
    pt = np.exp(tl64 - lse)
    dt_b = np.abs(coef) * (pt * (e_lse + 2 * U * np.abs(tl64 - lse) + 3 * U) + 2.0 ** -125) + 3 * U * np.abs(ref["dt"])
    for q, r in enumerate(ranks):
        loss, dX, dtq = out[q]
        n_tot = len(r["cols"]); own = slice(pre[q], pre[q + 1])
        note("ss_finish loss", abs(loss - ref["loss"][q]),
             term_b[own].sum() + (pre[q + 1] - pre[q] + 1) * U * (np.abs(ref["term"][own]).sum() + 1.5) + 1e-300)
        note("ss_finish dt", np.abs(dtq[:nlive] - ref["dt"]), dt_b)
        assert np.all(dtq[nlive:npad] == 0) and np.all(dtq[npad:] == SENT)
        assert np.all(dX[:nlive, n_tot:] == 0) and np.all(dX[nlive:npad] == 0) and np.all(dX[npad:] == SENT)
        if n_tot == 0:
            continue
        d = ref["dl"][q]
        w = sn.ss_weights(r["len"], r["n_s"], n_tot)
        xl = np.where(ref["act"][q], r["X"] - lse[:, None], 0.0)
        p = np.exp(xl)
        bound = np.abs(coef)[:, None] * w[None, :] * (p * (e_lse[:, None] + 2 * U * np.abs(xl) + 3 * U) + 2.0 ** -125) + 4 * U * np.abs(d)
        if dt == BF16:
            bound = bound + bf16_ulp(d)
        note("ss_finish dlogits", np.abs(dX[:nlive, :n_tot] - d), np.where(ref["act"][q], bound, 0.0))   # inactive entries: exactly zero
        for (qq, row, c) in hit_slots:
            if qq == q:
                assert dX[row, c] == 0 and not ref["act"][q][row, c]
        for (qq, c) in drop_slots:
            if qq == q:
                assert np.all(dX[:nlive, c] == 0)
    if det:
        again = run()[4]
        assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(out, again))


# ============================================================================================ ss_target_grad
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("nlive,D", [(1, 64), (64, 136), (65, 512), (130, 520), (200, 2048)])
def test_ss_target_grad(dev, dt, det, nlive, D):
    rng = np.random.default_rng(nlive + D)
    length, col0, rows = 23, 300, nlive + 5
    loc = rng.integers(6, length, rows)                                           # classes 0 .. 5 are placed by hand below
    g = rng.standard_normal(rows).astype(np.float32)
    for r, c in ((3, 0), (70, 0), (199, 0),                                       # a class shared across the 64-row blocks
                 (66, 1), (100, 1),                                               # a class whose first row lies in the second block
                 (5, 2), (80, 2), (64, 2),                                        # a class whose FIRST row has dt = 0
                 (7, -1), (8, length), (9, -col0), (63, 3), (129, 4)):            # out of range: a neighbour's, far away
        if r < rows:
            loc[r] = c
    for r in (5, 11, 68):
        if r < nlive:
            g[r] = 0.0
    # the stale rows behind nlive name the class of the last live row, with dt != 0: the sweep over that row's 64-row block must stop at
    # nlive, or fp64 shows their terms.  Class 5 has no row at all.
    loc[nlive:] = loc[nlive - 1]
    assert 0 <= loc[nlive - 1] < length and g[nlive - 1] != 0 and np.all(g[nlive:] != 0) and not np.any(loc == 5)
    Ew = storage(rng.standard_normal((rows, D)), dt); Fl = storage(rng.standard_normal((length, D)), dt)
    gE0 = rng.standard_normal((length, D)).astype(np.float32); dE0 = rng.standard_normal((rows, D)).astype(np.float32)
    dM = dev.put(meta_rows(loc + col0, np.ones(rows), np.ones(rows)))

    def run():
        dg, de = dev.put(gE0), dev.put(dE0)
        _ok(ss_call(dev, dt, 1024, det=det, length=length, col0=col0, metaC=dM, nlive=dev.puti([nlive]), rows=nlive, EwC=dev.put(Ew, dt),
                    Floc=dev.put(Fl, dt), D=D, dt_=dev.put(g), gE=dg, dEwC=de))
        return dev.get(dg, (length, D)), dev.get(de, (rows, D))

    gE, dE = run()
    dF, dFmag, dEadd, cnt = sn.ss_target_grad(Ew[:nlive], Fl, loc[:nlive], g[:nlive].astype(np.float64), length)
    k = cnt[:, None]
    note("ss_target_grad dF", np.abs(gE - (gE0 + dF)), (2 * k + 2) * U * (np.abs(gE0) + dFmag))
    note("ss_target_grad dEw", np.abs(dE[:nlive] - (dE0[:nlive] + dEadd)), 2 * U * (np.abs(dE0[:nlive]) + np.abs(dEadd)))
    live = np.zeros(length, bool); ok = (loc[:nlive] >= 0) & (loc[:nlive] < length) & (g[:nlive] != 0); live[loc[:nlive][ok]] = True
    assert np.array_equal(gE[~live], gE0[~live])                                  # class rows without a live target: untouched
    assert np.array_equal(dE[nlive:], dE0[nlive:])
    untouched = ~ok
    assert np.array_equal(dE[:nlive][untouched], dE0[:nlive][untouched])          # rows with dt = 0 or a foreign target: untouched
    if det:
        gE2, dE2 = run()
        assert np.array_equal(gE, gE2) and np.array_equal(dE, dE2)
