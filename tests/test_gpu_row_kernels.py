"""GPU: the row kernels between the products and the optimiser, one launch at a time through their C-ABI hooks (rsys_debug.h):
RMSNorm forward / backward (every template instance), the cross entropy of the tied heads, the rating-head tail, the gradient sum of
squares and clip + AdamW.  Each is compared with a float64 restatement of the same operation on the same (storage-rounded) inputs.

Bounds are derived, not tuned (u = 2^-24, the fp32 unit roundoff):
- an fp32 result is within c u of the fp64 value, scaled by the sum of the magnitudes of the terms that went into it, where c counts
  the roundings on the longest chain of the kernel's summation order (written next to each assertion);
- a bf16-stored result is within one bf16 ulp of the fp64 value (the fp32 value it is rounded from is within a few fp32 ulp);
- rows and columns a kernel must not touch are filled with a sentinel first, and every output buffer has a guard tail after it.
Deterministic mode (per-workgroup partials added in a fixed order) must give two bitwise equal launches, each within the same bound
as the default mode; the hooks fail if the launch did not take the partial-sum branch."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT = -7.5          # sentinel: exact in fp32 and bf16
GUARD = 64           # guard elements after every output buffer
F32, BF16 = 0, 1
DTYPES = [F32, BF16]


def _lib():
    from recommendersystem_amd import _lib
    return _lib


def bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + ((u >> 16) & 1) + 0x7FFF) & 0xFFFF0000).view(np.float32)


def bf16_ulp(x):
    """the spacing of bf16 numbers at |x| (8 significant bits)"""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return np.exp2(np.floor(np.log2(a)) - 7)


def storage(x, dt):
    """the value a T-typed buffer holds for x"""
    return bf16_round(x) if dt == BF16 else np.asarray(x, np.float32)


class Dev:
    """device buffers of one test: put() uploads (with a sentinel guard tail), get() reads back and checks the guard"""

    def __init__(self):
        self.L = _lib().lib()
        self.bufs = []

    def _raw(self, nbytes):
        p = C.c_void_p()
        assert self.L.rsys_dev_alloc(C.byref(p), nbytes) == 0, _lib().last_error()
        self.bufs.append(p)
        return p

    def put(self, arr, dt=None):
        """float arrays are stored as fp32, or as bf16 when dt == BF16; int arrays as int32"""
        a = np.asarray(arr)
        if a.dtype.kind in "iu":
            h = np.concatenate([a.ravel().astype(np.int32), np.full(GUARD, -12345, np.int32)])
        elif dt == BF16:
            h = np.concatenate([bf16_round(a.ravel()).view(np.uint32) >> 16, np.full(GUARD, 0xC0F0, np.uint32)]).astype(np.uint16)
        else:
            h = np.concatenate([a.ravel().astype(np.float32), np.full(GUARD, SENT, np.float32)])
        p = self._raw(h.nbytes)
        assert self.L.rsys_dev_h2d(p, h.ctypes.data, h.nbytes) == 0
        return p

    def get(self, p, shape, dt=None):
        """read back a float buffer put() made (fp32, or bf16 widened); asserts that its guard tail is untouched"""
        n = int(np.prod(shape))
        h = np.empty(n + GUARD, np.uint16 if dt == BF16 else np.float32)
        assert self.L.rsys_dev_d2h(h.ctypes.data, p, h.nbytes) == 0
        if dt == BF16:
            h = (h.astype(np.uint32) << 16).view(np.float32)
        assert np.all(h[n:] == SENT), "write past the end of the buffer"
        return h[:n].reshape(shape)

    def free(self):
        for p in self.bufs:
            self.L.rsys_dev_free(p)
        self.bufs = []


@pytest.fixture
def dev():
    d = Dev()
    yield d
    d.free()


def _ok(rc):
    assert rc == 0, _lib().last_error()


# ============================================================================================ RMSNorm
NORM_D = [64, 192, 256, 320, 512, 768, 1024, 1536, 2048]   # every (NJ, EXACT) instance: NJ = 1, 2, 4, 8, exact and not


def _nj(D):
    return max(1, -(-D // 256))


def _rmsnorm64(x, s):
    r = 1.0 / np.sqrt((x * x).mean(-1, keepdims=True) + 1e-5)
    return x * r * s, r[:, 0]


def _fwd_bound(y_ref, D):
    # sum of squares: a lane adds 4 NJ squares in a chain, then a 6-level wave tree (+1 for the square): rel. error (4 NJ + 7) u;
    # / D, + eps, rsqrt: 3 u more; r has half the relative error of its argument; y = x r s: 2 roundings
    return (0.5 * (4 * _nj(D) + 10) + 4) * U * np.abs(y_ref)


def _run_fwd(dev, dt, x, s, rows_cap=None, rows_dev=None, in_rows=None, amax=False):
    rows, D = x.shape
    cap = rows if rows_cap is None else rows_cap
    dx = dev.put(x); ds = dev.put(s)
    dy = dev.put(np.full((cap, D), SENT, np.float32), dt); dr = dev.put(np.full(cap, SENT, np.float32))
    drows = dev.put(np.array([rows_dev], np.int32)) if rows_dev is not None else None
    dperm = dev.put(np.asarray(in_rows, np.int32)) if in_rows is not None else None
    dam = dev.put(np.zeros(64 * 32, np.float32)) if amax else None
    _ok(dev.L.rsys_op_rmsnorm_fwd(dt, dx, ds, dy, dr, cap, D, drows, dperm, dam))
    y = dev.get(dy, (cap, D), dt); r = dev.get(dr, (cap,))
    am = dev.get(dam, (64, 32))[:, 0].max() if amax else None
    return y, r, am


def _check_fwd(y, r, x, s, dt):
    D = x.shape[1]
    y_ref, r_ref = _rmsnorm64(x.astype(np.float64), s.astype(np.float64))
    assert np.all(np.abs(r - r_ref) <= (0.5 * (4 * _nj(D) + 10) + 2) * U * r_ref), np.abs(r / r_ref - 1).max()
    if dt == F32:
        err = np.abs(y - y_ref) - _fwd_bound(y_ref, D)
    else:   # the fp32 value is within the bound above of y_ref: its bf16 rounding is within one bf16 ulp of y_ref
        err = np.abs(y - y_ref) - bf16_ulp(y_ref)
    assert err.max() <= 0, (float(err.max()), np.unravel_index(np.argmax(err), err.shape))


@pytest.mark.parametrize("D", NORM_D)
@pytest.mark.parametrize("dt", DTYPES)
def test_rmsnorm_fwd(dev, dt, D):
    rng = np.random.default_rng(D + 7 * dt)
    s = (1.0 + 0.3 * rng.standard_normal(D)).astype(np.float32)
    for rows, mag in [(1, 1.0), (3, 1e-3), (37, 1e3), (130, 1.0)]:
        # (1e-3: mean x^2 ~ 1e-6, the eps 1e-5 inside the rsqrt dominates; 1e3: it is invisible)
        x = (mag * rng.standard_normal((rows, D))).astype(np.float32)
        y, r, am = _run_fwd(dev, dt, x, s, amax=True)
        _check_fwd(y, r, x, s, dt)
        assert am == np.abs(y).max()   # the amax of the stored (rounded) values, exactly


@pytest.mark.parametrize("D", [192, 1024])
@pytest.mark.parametrize("dt", DTYPES)
def test_rmsnorm_fwd_compact_rows_and_permuted_input(dev, dt, D):
    rng = np.random.default_rng(3)
    s = (1.0 + 0.3 * rng.standard_normal(D)).astype(np.float32)
    cap = 600                                   # > every n rounded up to 256 below
    x = rng.standard_normal((cap, D)).astype(np.float32)
    for n in (0, 1, 255, 256, 257):
        y, r, _ = _run_fwd(dev, dt, x, s, rows_cap=cap, rows_dev=n)
        z = min(cap, (n + 255) // 256 * 256)
        if n:
            _check_fwd(y[:n], r[:n], x[:n], s, dt)
        assert np.all(y[n:z] == 0) and np.all(r[n:z] == 0), n      # rows n .. round-up-256: exactly zero
        assert np.all(y[z:] == SENT) and np.all(r[z:] == SENT), n  # rows past that: untouched
    perm = rng.permutation(cap).astype(np.int32)
    y, r, _ = _run_fwd(dev, dt, x, s, in_rows=perm)
    _check_fwd(y, r, x[perm], s, dt)


# ---------------------------------------------------------------------------- backward
def _bwd_ref(g, x, s, r, resid):
    """fp64 backward on the stored inputs, plus the magnitudes the bounds scale with"""
    D = x.shape[1]
    gs = g * s
    dot = (gs * x).sum(1, keepdims=True)
    dx = r[:, None] * gs - x * (r[:, None] ** 3) * dot / D + resid
    mag = np.abs(r[:, None] * gs) + np.abs(x) * (r[:, None] ** 3) * np.abs(gs * x).sum(1, keepdims=True) / D + np.abs(resid)
    terms = g * x * r[:, None]
    return dx, mag, terms.sum(0), np.abs(terms).sum(0)


def _run_bwd(dev, dt, g, x, s, r, det, resid=None, resid_slot=None, io_rows=None, rows_dev=None, g_f32=False, rows_cap=None):
    rows, D = g.shape
    cap = rows if rows_cap is None else rows_cap
    dg = dev.put(g, F32 if g_f32 else dt); dxin = dev.put(x); dsc = dev.put(s); drs = dev.put(r)
    dres = dev.put(resid) if resid is not None else None
    dslot = dev.put(resid_slot) if resid_slot is not None else None
    dio = dev.put(io_rows) if io_rows is not None else None
    drows = dev.put(np.array([rows_dev], np.int32)) if rows_dev is not None else None
    ddx = dev.put(np.full((cap, D), SENT, np.float32)); ddt = dev.put(np.full((cap, D), SENT, np.float32), dt)
    dds = dev.put(np.zeros(D, np.float32)); dam = dev.put(np.zeros(64 * 32, np.float32))
    _ok(dev.L.rsys_op_rmsnorm_bwd(dt, int(g_f32), dg, dxin, dsc, drs, dres, dslot, dio, drows, ddx, ddt, dds, cap, D, dam, int(det)))
    return dev.get(ddx, (cap, D)), dev.get(ddt, (cap, D), dt), dev.get(dds, (D,)), dev.get(dam, (64, 32))[:, 0].max()


def _check_bwd(dx, dxt, dscale, am, ref, dt, D, rows):
    dx_ref, mag, ds_ref, ds_mag = ref
    nj = _nj(D)
    # dx: the row dot product is a chain of 4 NJ products per lane and a 6-level wave tree; then r^3 dot / D and two fused terms
    err = np.abs(dx - dx_ref) - (4 * nj + 16) * U * mag
    assert err.max() <= 0, (float(err.max()), np.unravel_index(np.argmax(err), err.shape))
    # the operand copy is the rounding of the fp32 dx, bit for bit
    assert np.array_equal(dxt, storage(dx, dt))
    assert am == np.abs(dxt).max()
    # dscale: one term per row, summed over the rows in a per-lane chain, across the waves of a workgroup, then across workgroups
    # (atomics or partial rows): sqrt(rows) + 8 roundings of the magnitudes' sum
    e = np.abs(dscale - ds_ref) - (math.sqrt(rows) + 8) * 4 * U * ds_mag
    assert e.max() <= 0, (float(e.max()), int(np.argmax(e)))


def _bwd_inputs(rng, rows, D, dt, mag=1.0):
    x = (mag * rng.standard_normal((rows, D))).astype(np.float32)
    s = (1.0 + 0.3 * rng.standard_normal(D)).astype(np.float32)
    g = storage(rng.standard_normal((rows, D)), dt)
    r = _rmsnorm64(x.astype(np.float64), 1.0)[1].astype(np.float32)
    return g, x, s, r


@pytest.mark.parametrize("D", NORM_D)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("det", [0, 1])
def test_rmsnorm_bwd(dev, dt, D, det):
    rng = np.random.default_rng(100 + D + 3 * dt)
    # 4100 rows: more than the grid cap (1024 x 4 waves) holds, so waves loop and the deterministic path reduces > 64 partial rows
    for rows, mag in [(1, 1.0), (3, 1e-3), (37, 1e3), (4100, 1.0)]:
        g, x, s, r = _bwd_inputs(rng, rows, D, dt, mag)
        resid = rng.standard_normal((rows, D)).astype(np.float32)
        ref = _bwd_ref(g.astype(np.float64), x.astype(np.float64), s.astype(np.float64), r.astype(np.float64), resid.astype(np.float64))
        out = _run_bwd(dev, dt, g, x, s, r, det, resid=resid)
        _check_bwd(*out, ref, dt, D, rows)
        if det:   # two launches, the same bits
            again = _run_bwd(dev, dt, g, x, s, r, det, resid=resid)
            assert all(np.array_equal(a, b) for a, b in zip(out[:3], again[:3]))
        # the final norm's form: an fp32 incoming gradient whatever the operand type
        gf = rng.standard_normal((rows, D)).astype(np.float32)
        ref = _bwd_ref(gf.astype(np.float64), x.astype(np.float64), s.astype(np.float64), r.astype(np.float64), 0.0 * resid)
        _check_bwd(*_run_bwd(dev, dt, gf, x, s, r, det, g_f32=True), ref, dt, D, rows)


@pytest.mark.parametrize("D", [192, 1024])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("det", [0, 1])
def test_rmsnorm_bwd_compact_rows_residual_slots_and_permutation(dev, dt, D, det):
    rng = np.random.default_rng(7)
    cap = 600
    g, x, s, r = _bwd_inputs(rng, cap, D, dt)
    g64, x64, s64, r64 = (a.astype(np.float64) for a in (g, x, s, r))
    for n in (0, 1, 255, 256, 257):
        dx, dxt, dscale, am = _run_bwd(dev, dt, g, x, s, r, det, rows_dev=n)
        z = min(cap, (n + 255) // 256 * 256)
        if n:
            ref = _bwd_ref(g64[:n], x64[:n], s64, r64[:n], 0.0)
            _check_bwd(dx[:n], dxt[:n], dscale, am, ref, dt, D, n)
        else:
            assert np.all(dscale == 0)
        assert np.all(dx[n:z] == 0) and np.all(dxt[n:z] == 0), n
        assert np.all(dx[z:] == SENT) and np.all(dxt[z:] == SENT), n
    # residual from a compact buffer through resid_slot (-1: none), x read / dx written at io_rows
    nres = 97
    resid = rng.standard_normal((nres, D)).astype(np.float32)
    slot = rng.integers(-1, nres, cap).astype(np.int32)
    slot[:5] = -1
    perm = rng.permutation(cap).astype(np.int32)
    dx, dxt, dscale, am = _run_bwd(dev, dt, g, x, s, r, det, resid=resid, resid_slot=slot, io_rows=perm)
    rr = np.where(slot[:, None] >= 0, resid[np.maximum(slot, 0)], 0.0)
    dx_ref, mag, ds_ref, ds_mag = _bwd_ref(g64, x64[perm], s64, r64, rr)
    _check_bwd(dx[perm], dxt[perm], dscale, am, (dx_ref, mag, ds_ref, ds_mag), dt, D, cap)
    # io_rows with rows_dev: rejected (the zero rows would land at unmapped rows)
    from recommendersystem_amd import _lib as L
    drows = dev.put(np.array([5], np.int32)); dio = dev.put(perm)
    buf = [dev.put(np.zeros((cap, D), np.float32)) for _ in range(6)]
    rc = dev.L.rsys_op_rmsnorm_bwd(F32, 0, buf[0], buf[1], buf[2], buf[3], None, None, dio, drows, buf[4], None, buf[5], cap, D, None, 0)
    assert rc != 0 and "io_rows" in L.last_error()


# ============================================================================================ cross entropy
def _ce_ref(X, V, idx, label, weight, pos, stats0, npos, task_w):
    """fp64 loss and dlogits of ce_kernel on the stored logits X [n][ldl], and per-element bounds (see test_ce)"""
    n, ldl = X.shape
    lim = n if npos is None else min(n, (npos + 127) // 128 * 128)
    loss = 0.0; loss_bound = 0.0
    dl = X.astype(np.float64).copy(); bound = np.zeros_like(dl)
    for row in range(lim):
        i = idx[row]
        lw = float(label[i]) * float(weight[i])
        if lw == 0.0:
            dl[row] = 0.0
            continue
        x = X[row, :V].astype(np.float64)
        gm = x.max()
        lse = gm + math.log(np.exp(x - gm).sum())
        # lse in fp32: the max is exact; the online sum is a chain of ceil(V / 256) exp-and-adds per thread (3 roundings each, __expf's
        # argument carries |gm| u) and two 8-level workgroup trees; log adds 2 u |lse|
        e_lse = U * (2 * abs(gm) + 2 * abs(lse) + 3 * -(-V // 256) + 32)
        t = pos[i]
        loss += (lse - x[t]) * lw
        loss_bound += (e_lse + 2 * U * abs(lse - x[t])) * abs(lw)
        coef = task_w * lw / max(stats0, 1e-8)
        p = np.exp(x - lse)
        d = p.copy(); d[t] -= 1.0
        dl[row, :V] = coef * d
        dl[row, V:] = 0.0
        # dlogit: exp(x - lse) carries (e_lse + 2 |x - lse| u + 3 u) relatively (__expf scales its argument by log2 e), the
        # subtraction and the product 3 u |result|; probabilities below the smallest normal fp32 may be flushed to zero
        bound[row, :V] = abs(coef) * (p * (e_lse + 2 * U * np.abs(x - lse) + 3 * U) + 2.0 ** -125) + 3 * U * np.abs(coef * d)
    # the rows' terms: summed in row order (deterministic) or by atomics: n roundings of the magnitudes' sum at most
    return loss, loss_bound + n * U * abs(loss), dl, bound, lim


def _run_ce(dev, dt, X, V, idx, label, weight, pos, stats0, npos, task_w, det):
    n, ldl = X.shape
    dX = dev.put(X, dt)
    di = dev.put(idx); dlab = dev.put(label); dw = dev.put(weight); dp = dev.put(pos)
    dst = dev.put(np.array([stats0, 0.0], np.float32))
    dn = dev.put(np.array([npos], np.int32)) if npos is not None else None
    dloss = dev.put(np.zeros(1, np.float32))
    _ok(dev.L.rsys_op_ce(dt, dX, ldl, n, V, di, dlab, dw, dp, dst, dn, C.c_float(task_w), dloss, int(det)))
    return float(dev.get(dloss, (1,))[0]), dev.get(dX, (n, ldl), dt)


def _ce_case(rng, dt, n, V, shift=0.0, pad=1e30, npos=None, peaked=False):
    ldl = (V + 1 + 7) // 8 * 8                            # > V, 16-byte rows in both types
    X = rng.standard_normal((n, ldl)) * 3.0 + shift
    X[:, V:] = pad
    N = n + 5
    idx = rng.permutation(N)[:n].astype(np.int32)
    label = rng.uniform(0.5, 1.5, N).astype(np.float32)
    weight = rng.uniform(0.2, 2.0, N).astype(np.float32)
    weight[idx[1::4]] = 0.0                                 # rows with label * weight = 0: cleared
    pos = rng.integers(0, V, N).astype(np.int32)
    pos[idx[0]] = 0; pos[idx[-1]] = V - 1                   # targets at both ends
    if peaked:   # the target holds nearly all the mass: lse - x_t ~ V e^-40
        for row in range(n):
            X[row, pos[idx[row]]] = shift + 40.0
    return storage(X, dt), idx, label, weight, pos


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("V", [1, 7, 8, 9, 4097, 200003])
def test_ce(dev, dt, det, V):
    rng = np.random.default_rng(V + 11 * dt)
    cases = [dict(), dict(shift=80.0, pad=float("nan")), dict(shift=-80.0), dict(shift=1e4), dict(shift=-1e4, pad=float("nan")),
             dict(peaked=True)]
    for k, case in enumerate(cases):
        n = 3 if V > 10000 else 13
        X, idx, label, weight, pos = _ce_case(rng, dt, n, V, **case)
        stats0 = float(rng.uniform(1.0, 5.0)) if k != 2 else 3e-9   # stats[0] below 1e-8: the divisor is 1e-8
        task_w = 0.3
        loss, dX = _run_ce(dev, dt, X, V, idx, label, weight, pos, stats0, None, task_w, det)
        l_ref, l_bound, dl_ref, bound, lim = _ce_ref(X, V, idx, label, weight, pos, stats0, None, task_w)
        assert abs(loss - l_ref) <= l_bound, (case, loss, l_ref, l_bound)
        if dt == F32:
            err = np.abs(dX - dl_ref) - bound
        else:   # one bf16 ulp of the fp64 value, plus the fp32 error where the value is a cancellation (p_t - 1 of a peaked row)
            err = np.abs(dX - dl_ref) - (bf16_ulp(dl_ref) + bound)
        assert err.max() <= 0, (case, float(err.max()), np.unravel_index(np.argmax(err), err.shape))
        assert np.all(dX[:, V:] == 0)                      # padding columns: no term, and a zero gradient
        if det:
            again = _run_ce(dev, dt, X, V, idx, label, weight, pos, stats0, None, task_w, det)
            assert again[0] == loss and np.array_equal(again[1], dX)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("det", [0, 1])
def test_ce_npos_rounding_and_empty_launch(dev, dt, det):
    rng = np.random.default_rng(5)
    V, n = 33, 300
    X, idx, label, weight, pos = _ce_case(rng, dt, n, V)
    for npos in (0, 5, 128, 129):
        loss, dX = _run_ce(dev, dt, X, V, idx, label, weight, pos, 2.0, npos, 0.3, det)
        l_ref, l_bound, dl_ref, bound, lim = _ce_ref(X, V, idx, label, weight, pos, 2.0, npos, 0.3)
        assert lim == min(n, (npos + 127) // 128 * 128)
        assert abs(loss - l_ref) <= l_bound, (npos, loss, l_ref)
        tol = bound[:lim] + (bf16_ulp(dl_ref[:lim]) if dt == BF16 else 0)
        assert np.all(np.abs(dX[:lim] - dl_ref[:lim]) <= tol), npos
        assert np.array_equal(dX[lim:], X[lim:], equal_nan=True), npos   # rows at or past round-up-128: untouched
    loss, dX = _run_ce(dev, dt, X[:0], V, idx, label, weight, pos, 2.0, None, 0.3, det)   # n = 0 launches nothing
    assert loss == 0.0


# ============================================================================================ rating tail
def _gelu_grad(z):
    return 0.5 * (1.0 + np.vectorize(math.erf)(z / math.sqrt(2.0))) + z * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def _tail_ref(z, h, w2, b2, idx, label, weight, stats0, mean, task_w, evaluate, npos):
    n, D = z.shape
    lim = n if npos is None else min(n, (npos + 127) // 128 * 128)
    z = z[:lim].astype(np.float64); h = h[:lim].astype(np.float64); w2 = w2.astype(np.float64)
    i = idx[:lim]
    wt = weight[i].astype(np.float64); t = label[i].astype(np.float64) - np.float64(np.float32(mean))
    pred = h @ w2 + float(b2)
    # pred: a lane's chain of D / 64 products, a 6-level wave tree and + b2
    e_pred = U * ((D // 64 + 8) * (np.abs(h) @ np.abs(w2)) + abs(float(b2)))
    e1 = pred - t
    # e1 and -pred - t also carry the rounding of t = label - mean and of their own subtraction
    e_e1 = e_pred + U * (np.abs(t) + np.abs(e1)); e_e2 = e_pred + U * (np.abs(t) + np.abs(pred + t))
    terms = [e1 * e1 * wt, t * t * wt, (pred + t) ** 2 * wt]
    loss = np.array([a.sum() for a in terms])
    e_terms = [2 * np.abs(e1 * wt) * e_e1 + 4 * U * np.abs(terms[0]),
               6 * U * np.abs(terms[1]),
               2 * np.abs((pred + t) * wt) * e_e2 + 4 * U * np.abs(terms[2])]
    # the rows' terms: a chain per wave over its rows, then waves and workgroups: rows + 8 roundings of the magnitudes' sum at most
    loss_bound = np.array([e.sum() + (lim + 8) * U * np.abs(a).sum() for a, e in zip(terms, e_terms)])
    k = 0.0 if evaluate else task_w * 2.0 / max(stats0, 1e-8)
    dpred = k * e1 * wt
    e_dpred = abs(k) * np.abs(wt) * e_e1 + 6 * U * np.abs(dpred)
    gp = _gelu_grad(z)
    zphi = z * np.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    # gelu'(z) = A + z phi(z) in fp32, A = (1 + erf(z / sqrt 2)) / 2: erff is within 2 ulp of |erf| -- an ABSOLUTE error where 1 + erf
    # cancels (z < 0) -- and the rounding of its argument moves it by |z| phi(z) u; 2 roundings of A.  __expf(-z^2 / 2) carries
    # 2 |z^2 / 2| u through its scaled argument, and 6 roundings of the second term
    e_gp = U * (4 * np.abs(2 * (gp - zphi) - 1) + 2 * np.abs(gp - zphi) + (z * z + 8) * np.abs(zphi))
    dz = dpred[:, None] * w2[None, :] * gp
    e_dz = np.abs(w2[None, :]) * (e_dpred[:, None] * np.abs(gp) + np.abs(dpred)[:, None] * e_gp) + 3 * U * np.abs(dz)
    dw2 = dpred @ h; e_dw2 = e_dpred @ np.abs(h) + (lim + 8) * U * (np.abs(dpred) @ np.abs(h))
    db0 = dz.sum(0); e_db0 = e_dz.sum(0) + (lim + 8) * U * np.abs(dz).sum(0)
    db2 = dpred.sum(); e_db2 = e_dpred.sum() + (lim + 8) * U * np.abs(dpred).sum()
    return lim, loss, loss_bound, dz, e_dz, dw2, e_dw2, db0, e_db0, db2, e_db2


def _run_tail(dev, dt, z, h, w2, b2, idx, label, weight, stats0, mean, task_w, evaluate, npos, det):
    n, D = z.shape
    dz = dev.put(z, dt); dh = dev.put(h, dt); dw2 = dev.put(w2); db2 = dev.put(np.array([b2], np.float32))
    di = dev.put(idx); dlab = dev.put(label); dwt = dev.put(weight); dst = dev.put(np.array([stats0, 0.0], np.float32))
    dn = dev.put(np.array([npos], np.int32)) if npos is not None else None
    dloss = dev.put(np.zeros(3, np.float32))
    gw2 = dev.put(np.zeros(D, np.float32)); gb2 = dev.put(np.zeros(1, np.float32)); gb0 = dev.put(np.zeros(D, np.float32))
    _ok(dev.L.rsys_op_rating_tail(dt, dz, dh, n, D, dw2, db2, di, dlab, dwt, dst, C.c_float(mean), C.c_float(task_w), int(evaluate),
                                  dloss, gw2, gb2, gb0, dn, int(det)))
    return (dev.get(dz, (n, D), dt), dev.get(dloss, (3,)), dev.get(gw2, (D,)), dev.get(gb0, (D,)), float(dev.get(gb2, (1,))[0]))


def _tail_case(rng, dt, n, D):
    z = storage(rng.uniform(-8.0, 8.0, (n, D)), dt)        # the GELU derivative over |z| <= 8
    h = storage(rng.standard_normal((n, D)) * 0.5, dt)
    w2 = (rng.standard_normal(D) / math.sqrt(D)).astype(np.float32)
    b2 = np.float32(0.3)
    N = n + 3
    idx = rng.permutation(N)[:n].astype(np.int32)
    label = rng.uniform(1.0, 10.0, N).astype(np.float32)
    weight = rng.uniform(-1.0, 2.0, N).astype(np.float32)  # negative weights
    weight[idx[2::5]] = 0.0                                 # and zero weights
    return z, h, w2, b2, idx, label, weight


def _check_tail(out, ref, dt):
    dz, loss, dw2, db0, db2 = out
    lim, l_ref, l_b, dz_ref, e_dz, dw2_ref, e_dw2, db0_ref, e_db0, db2_ref, e_db2 = ref
    assert np.all(np.abs(loss - l_ref) <= l_b), (loss, l_ref, l_b)
    tol = e_dz + (bf16_ulp(dz_ref) if dt == BF16 else 0.0)
    err = np.abs(dz[:lim] - dz_ref) - tol
    assert err.max() <= 0, (float(err.max()), np.unravel_index(np.argmax(err), err.shape))
    assert np.all(np.abs(dw2 - dw2_ref) <= e_dw2), float((np.abs(dw2 - dw2_ref) - e_dw2).max())
    assert np.all(np.abs(db0 - db0_ref) <= e_db0), float((np.abs(db0 - db0_ref) - e_db0).max())
    assert abs(db2 - db2_ref) <= e_db2, (db2, db2_ref, e_db2)


@pytest.mark.parametrize("D", [64, 192, 512, 1024, 2048])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("det", [0, 1])
def test_rating_tail(dev, dt, D, det):
    # (D = 2048 in deterministic mode takes 8 D + 16 floats = 65 600 bytes of dynamic LDS)
    rng = np.random.default_rng(D + 5 * dt)
    mean = 3.25
    for n, evaluate, npos in [(1, 0, None), (7, 0, None), (130, 0, 3), (130, 1, None), (2100, 0, None)]:
        # 2100 rows > 512 workgroups x 4 waves: the grid is capped and the waves loop
        z, h, w2, b2, idx, label, weight = _tail_case(rng, dt, n, D)
        stats0 = float(np.abs(weight).sum()) if n != 7 else 1e-12    # stats[0] below 1e-8: the divisor is 1e-8
        out = _run_tail(dev, dt, z, h, w2, b2, idx, label, weight, stats0, mean, 0.25, evaluate, npos, det)
        ref = _tail_ref(z, h, w2, b2, idx, label, weight, stats0, mean, 0.25, evaluate, npos)
        _check_tail(out, ref, dt)
        lim = ref[0]
        assert np.array_equal(out[0][lim:], z[lim:]), "rows past round-up-128 of npos must be untouched"
        if evaluate:
            assert np.all(out[2] == 0) and np.all(out[3] == 0) and out[4] == 0
        if det:
            again = _run_tail(dev, dt, z, h, w2, b2, idx, label, weight, stats0, mean, 0.25, evaluate, npos, det)
            assert all(np.array_equal(a, b) for a, b in zip(out, again))


def test_rating_tail_empty_launch(dev):
    z, h, w2, b2, idx, label, weight = _tail_case(np.random.default_rng(1), F32, 4, 64)
    for det in (0, 1):
        dz, loss, dw2, db0, db2 = _run_tail(dev, F32, z[:0], h[:0], w2, b2, idx, label, weight, 1.0, 0.0, 1.0, 0, None, det)
        assert np.all(loss == 0) and np.all(dw2 == 0) and np.all(db0 == 0) and db2 == 0


# ============================================================================================ sum of squares, clip + AdamW
@pytest.mark.parametrize("n", [1, 3, 1001, 4097, 8_400_003])
def test_sumsq(dev, n):
    # 8 400 003: > 2047 * 1024 float4s, all 2048 partial sums; n % 4 != 0: the tail goes to workgroup 0's extra loop
    rng = np.random.default_rng(n)
    g = rng.standard_normal(n).astype(np.float32)
    g[-(n % 4 or 1):] = 1e3                                   # the tail dominates: dropping it is visible
    dg = dev.put(g); out = dev.put(np.zeros(1, np.float32))
    _ok(dev.L.rsys_op_sumsq(dg, n, out))
    s = float(dev.get(out, (1,))[0])
    ref = float((g.astype(np.float64) ** 2).sum())
    grid = min(((n >> 2) + 1023) // 1024 + 1, 2048)
    # all terms positive: the longest chain bounds the error.  A thread's float4s (5 roundings each into one accumulator), 2 to join
    # its accumulators and the tail, the 8-level workgroup tree, 8 partials per thread of the final pass and its tree
    chain = 5 * -(-(n >> 2) // (grid * 256)) + 2 + 8 + 8 + 8
    assert abs(s - ref) <= (chain + 2) * U * ref, (s, ref)
    _ok(dev.L.rsys_op_sumsq(dg, n, out))
    assert float(dev.get(out, (1,))[0]) == s                  # fixed order: the same bits again


def _adamw_ref(p, g, m, v, n_decay, lr, b1, b2, eps, wd, step, max_norm, grad_div):
    f = lambda a: np.float64(np.float32(a))                   # the kernel's parameters are fp32
    lr, b1, b2, eps, wd = f(lr), f(b1), f(b2), f(eps), f(wd)
    ss = float((g.astype(np.float64) ** 2).sum())
    inv = 1.0 / grad_div
    clip = max_norm > 0 and max_norm / (math.sqrt(ss) * inv + 1e-6) < 1.0
    coef = inv * (max_norm / (math.sqrt(ss) * inv + 1e-6) if clip else 1.0)
    # coef in fp32: sumsq's chain (<= 64 roundings at these sizes, halved by the sqrt) when clipping, then 4 roundings
    crel = U * ((32 if clip else 0) + 4)
    g64 = g.astype(np.float64) * coef
    decay = np.where(np.arange(p.size) < n_decay, 1.0 - lr * wd, 1.0)
    m1 = b1 * m + (1 - b1) * g64
    v1 = b2 * v + (1 - b2) * g64 * g64
    bc1 = 1 - b1 ** step; bc2s = math.sqrt(1 - b2 ** step)
    den = np.sqrt(v1) / bc2s + eps
    upd = (lr / bc1) * (m1 / den)
    p1 = p * decay - upd
    e_m = U * (2 * np.abs(b1 * m) + 3 * np.abs((1 - b1) * g64)) + np.abs((1 - b1) * g64) * crel
    e_v = U * (2 * np.abs(b2 * v) + 4 * np.abs((1 - b2) * g64 * g64)) + np.abs((1 - b2) * g64 * g64) * 2 * crel
    # the bias corrections 1 - powf(b, step) (powf within 2 ulp of b^step) and the sqrt: relative error of either
    e_bc = U * (4 + 2 * max(b1 ** step / bc1, b2 ** step / (1 - b2 ** step)))
    e_den = (0.5 * e_v / np.maximum(v1, 1e-300) * np.sqrt(v1) / bc2s) + U * 4 * den + e_bc * np.sqrt(v1) / bc2s
    e_p = U * 3 * np.abs(p * decay) + (lr / bc1) * (e_m / den + np.abs(m1) * e_den / den ** 2) + np.abs(upd) * (e_bc + 4 * U)
    return p1, m1, v1, e_p, e_m, e_v, coef, crel, ss


ADAM = dict(lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.1)


def _run_adamw(dev, dt, p, g, m, v, n_decay, step, max_norm, grad_div, zero_grad, skip, fused):
    n = p.size
    dp, dg, dm, dv = dev.put(p), dev.put(g), dev.put(m), dev.put(v)
    dsh = dev.put(np.full(n, SENT, np.float32), BF16) if dt == BF16 else None
    dss = dev.put(np.zeros(1, np.float32))
    a = ADAM
    rc = dev.L.rsys_op_clip_adamw(dt, dp, dg, dm, dv, dsh, n_decay, n, C.c_float(a["lr"]), C.c_float(a["b1"]), C.c_float(a["b2"]),
                                  C.c_float(a["eps"]), C.c_float(a["wd"]), step, C.c_float(max_norm), C.c_float(grad_div), int(zero_grad),
                                  skip[0], skip[1], int(fused), dss)
    if rc:
        return rc
    sh = dev.get(dsh, (n,), BF16) if dt == BF16 else None
    return dev.get(dp, (n,)), dev.get(dg, (n,)), dev.get(dm, (n,)), dev.get(dv, (n,)), sh, float(dev.get(dss, (1,))[0])


@pytest.mark.parametrize("plain", [0, 1])
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("dt", DTYPES)
def test_clip_adamw(dev, monkeypatch, dt, fused, plain):
    # RSYS_DEBUG_ADAMW bit 0: the plain-load form of adamw_kernel instead of the nontemporal one
    monkeypatch.setenv("RSYS_DEBUG_ADAMW", str(plain))
    rng = np.random.default_rng(17 + 2 * dt + fused + 4 * plain)
    n = 1024 * 37 + 12                                        # not a multiple of 1024 (one workgroup's 256 float4s)
    n_decay = 1024 * 20 + 520                                 # a float4 boundary in the middle of workgroup 20's range
    skip = (1024 * 9 + 4, 1024 * 30 + 16)
    cases = [(1, 1.0, 1.0, 1), (1000, 1.0, 1.0, 0), (1, 1e6, 2.0, 1), (1000, 0.0, 3.0, 0), (3, 5.0, 3.0, 1), (1000, 1e6, 1.0, 1)]
    for step, max_norm, grad_div, zero_grad in cases:
        # |g| ~ 0.5 sqrt(n) ~ 100: max_norm 1 and 5 clip, 1e6 does not, 0 turns the clip off
        p = rng.standard_normal(n).astype(np.float32)
        g = (0.5 * rng.standard_normal(n)).astype(np.float32)
        if step == 1:
            m = np.zeros(n, np.float32); v = np.zeros(n, np.float32)
        else:   # a running state, so the step depends on the gradient's scale (the first step is ~lr sign(g) whatever it is)
            m = (0.05 * rng.standard_normal(n)).astype(np.float32); v = (0.01 * rng.uniform(0.1, 1.0, n)).astype(np.float32)
        out = _run_adamw(dev, dt, p, g, m, v, n_decay, step, max_norm, grad_div, zero_grad, skip, fused)
        assert not isinstance(out, int), _lib().last_error()
        p1, g1, m1, v1, sh, ss = out
        p_ref, m_ref, v_ref, e_p, e_m, e_v, coef, crel, ss_ref = _adamw_ref(p, g, m, v, n_decay, step=step, max_norm=max_norm,
                                                                             grad_div=grad_div, **ADAM)
        case = (step, max_norm, grad_div, zero_grad)
        assert abs(ss - ss_ref) <= 64 * U * ss_ref, (case, ss, ss_ref)
        for name, a, ref, e in (("m", m1, m_ref, e_m), ("v", v1, v_ref, e_v), ("p", p1, p_ref, e_p)):
            err = np.abs(a - ref) - e
            assert err.max() <= 0, (case, name, float(err.max()), int(np.argmax(err)))
        if zero_grad:
            assert np.all(g1 == 0)
        elif fused:
            assert np.array_equal(g1, g)
        else:   # the scale pass left g * coef behind
            assert np.all(np.abs(g1 - g * coef) <= (U + crel) * np.abs(g * coef))
        if dt == BF16:   # the shadow is the bf16 rounding of the new parameters, except in the skip range
            inside = (np.arange(n) >= skip[0]) & (np.arange(n) < skip[1])
            assert np.array_equal(sh[~inside], bf16_round(p1)[~inside])
            assert np.all(sh[inside] == SENT)


def test_adamw_rejects_unaligned_decay_boundary(dev):
    from recommendersystem_amd import _lib as L
    n = 4096
    z = np.zeros(n, np.float32)
    rc = _run_adamw(dev, F32, z, z, z, z, 1027, 1, 1.0, 1.0, 0, (0, 0), 1)
    assert rc != 0 and "multiples of 4" in L.last_error()


@pytest.mark.parametrize("plain", [0, 1])
def test_adamw_grid_stride(dev, monkeypatch, plain):
    # more float4s than the 4096 x 256 threads of the grid: the grid-stride loop, and the decay boundary past the first sweep
    monkeypatch.setenv("RSYS_DEBUG_ADAMW", str(plain))
    rng = np.random.default_rng(99)
    n = 4 * 4096 * 256 + 4 * 1000 + 8
    n_decay = 4 * 4096 * 256 + 2000
    p = rng.standard_normal(n).astype(np.float32)
    g = (0.5 * rng.standard_normal(n)).astype(np.float32)
    m = (0.05 * rng.standard_normal(n)).astype(np.float32); v = (0.01 * rng.uniform(0.1, 1.0, n)).astype(np.float32)
    p1, g1, m1, v1, sh, ss = _run_adamw(dev, BF16, p, g, m, v, n_decay, 10, 1e6, 1.0, 1, (0, 0), 1)
    p_ref, m_ref, v_ref, e_p, e_m, e_v, coef, crel, ss_ref = _adamw_ref(p, g, m, v, n_decay, step=10, max_norm=1e6, grad_div=1.0, **ADAM)
    assert np.all(np.abs(p1 - p_ref) <= e_p) and np.all(np.abs(m1 - m_ref) <= e_m) and np.all(np.abs(v1 - v_ref) <= e_v)
    assert np.array_equal(sh, bf16_round(p1)) and np.all(g1 == 0)
