"""GPU: every fused GEMM epilogue (GemmEpi, csrc/gemm.hpp) on every kernel family that implements it, one launch at a time through
rsys_op_gemm_epi (rsys_debug.h), against a float64 restatement of the epilogue's definition on the same storage-rounded inputs.

Three pieces of code implement the epilogues: epi_item (gemm_epi.hpp) with the SwiGLU product loop of gemm.hip -- the LDS-staged form of
the 128x128 kernel, fp32 and bf16, row-major or K-major B; epilogue_regs (gemm_epi_reg.hpp) -- the register form of gemm8p and gemm8c with
its FULL-tile and edge-tile paths, the permlane16_swap pair store and the operand pipeline; and the same with four row blocks in gemm8c's
HALF form (128 x 256 tiles).  Every call reports the kernel that ran and whether gemm8c took its HALF form, and every case asserts both:
a forced kernel that is not eligible falls back to the 128x128 one without a word.

Which (epilogue x family) combinations exist -- `eligible` below restates the routing; a combination it leaves out is ruled out by:
  gemm8p, gemm8c (both forms), fp32 dtype or K-major B    gemm_route (gemm.hip): `if (!is_bf16<CT>::value || a_f32 || b_f32) return fallback`, and
                                          pick_rowmajor_kernel is asked only under `if (!a_km && !b_km)`
  gemm8p, accum = 1                       gemm8p_eligible (gemm8p.hip): `p.splitk > 1 || p.epi == EPI_ATOMIC || p.k_dev != nullptr || p.accum`
  gemm8p, RoPE with alpha != 1 or without rope_cs          gemm8p_eligible: `p.epi == EPI_QKV_ROPE && (p.alpha != 1.f || p.rope_cs == nullptr)`
  gemm8c, bias and GELU                   gemm8c_eligible (gemm8c.hip): the `default: return false` of its epilogue switch
  gemm8c, store with alpha != 1           gemm8c_eligible: `case EPI_STORE: return p.alpha == 1.f`
  gemm8c, RoPE with rope_pos or c_f32     gemm8c_eligible: `case EPI_QKV_ROPE: return p.rope_pos == nullptr && !p.c_f32`
  gemm8c HALF, accumulate and table       c8_half_class (gemm8c.hip): the `default: return false` of its switch
  gemm8c HALF, store with c_f32           c8_half_class: `case EPI_STORE: return !p.c_f32`
(EPI_ATOMIC, the split-K and K-major-A kernels belong to test_gpu_ops.py, the fp8 fields to test_gpu_fp8_*.py, the grouped kernels and
the fp8 split-K form to test_gpu_gemm_group.py.)

Exactness first.  Small-integer operands make the accumulators exact integers, and every epilogue operand (bias, residual, E, prior C,
alpha in {1, 2, 0.5}) is a small dyadic number: store, accumulate, bias, residual and table results are then exact in fp32 and must be
bit equal to the reference (bf16 outputs: to its bf16 rounding).  RoPE gets "tables" whose row 0 is (1, 0) and whose other entries are
drawn per (position, pair) from {0, +-1, +-0.5, +-0.25}: the kernel only does the arithmetic, so a wrong position, pair, head offset or
q / k / v boundary changes bits.  The SwiGLU [a|b] copy and the GELU z are exact too (power-of-two scaled integers).

Bounds of the inexact results are derived, not tuned (U = 2^-24; conventions of test_gpu_row_kernels.py):
- linear epilogues: one rounding per addition / multiplication of the epilogue, each U times the sum of the magnitudes that went into it;
- RoPE: 3 roundings per element, 3 U (|v0 c| + |v1 s|) (alpha is a power of two: exact); with accum one more for the addition;
- random operands only: the accumulation order of the K products may differ from fp64's by K U sum|a b| (`slack`), propagated through
  the epilogue's derivative; integer data has none;
- sigmoid from __expf and a reciprocal or division: relative error (|a| + 8) U -- the exponent-argument product (one rounding amplified
  by |a|), the 1-ulp hardware exp and rcp, the add, and the two or three multiplies around it; accumulators are kept in |a| <= 8;
- GELU: erff within 2 ulp of |erf| -- an absolute error where 1 + erf cancels -- plus the rounding of its argument (as derived for the
  rating tail in test_gpu_row_kernels.py);
- a bf16-stored value: the fp32 bound plus one bf16 ulp of the fp64 value.
Each check prints the largest error as a fraction of its bound (`pytest -s`).

Every output has leading dimensions strictly larger than its width (ldc, ldc2, ldr all different; EPI_SWIGLU_BWD must have ldc2 == ldc
and EPI_TABLE reads E with ldc), is pre-filled with a sentinel, and must come back unchanged outside [M][width], padding columns and a
guard tail included."""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_row_kernels import BF16, F32, SENT, U, _lib, bf16_round, bf16_ulp, dev, storage  # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu

STORE, ACCUM, BIAS, RESID, ROPE, SWIGLU, TABLE, GELU, SWIGLU_BWD = 0, 1, 3, 4, 5, 6, 7, 8, 9
EPI_NAMES = {STORE: "store", ACCUM: "accum", BIAS: "bias", RESID: "resid", ROPE: "rope", SWIGLU: "swiglu", TABLE: "table", GELU: "gelu",
             SWIGLU_BWD: "swiglu_bwd"}
LIM = 8.0   # |a| of the sigmoid / GELU arguments

# family -> (switches, rows per output tile, HALF flag).  The tag is "8p" / "8c", or "nt" / "nn" (row-major / K-major B) for the 128x128 kernel
FAMILIES = {
    "128": ({"RSYS_GEMM_KERNEL": "1"}, 128, 0),
    "8p": ({"RSYS_GEMM_KERNEL": "2", "RSYS_GEMM8C": "0"}, 256, 0),
    "8c": ({"RSYS_GEMM_KERNEL": "2", "RSYS_GEMM8C": "1", "RSYS_GEMM8C_HALF": "0"}, 256, 0),
    "8ch": ({"RSYS_GEMM_KERNEL": "2", "RSYS_GEMM8C": "1", "RSYS_GEMM8C_HALF": "2"}, 128, 1),
}
FAM256 = ("8p", "8c", "8ch")
# (family, dtype, b_km) the families are run in: the 128x128 kernel in both dtypes with both B layouts, the 256 family in bf16, row-major
CONFIGS = [("128", F32, 0), ("128", F32, 1), ("128", BF16, 0), ("128", BF16, 1), ("8p", BF16, 0), ("8c", BF16, 0), ("8ch", BF16, 0)]
SWITCHES = ("RSYS_GEMM_KERNEL", "RSYS_GEMM8C", "RSYS_GEMM8C_HALF", "RSYS_GEMM4P", "RSYS_GEMM_PATCH", "RSYS_GEMM_REVERSE", "RSYS_DEBUG_8P",
            "RSYS_DEBUG_EPI", "RSYS_GEMM_KERNEL_NT_SPLITK")


def eligible(fam, dt, b_km, epi, c_f32=0, alpha=1.0, accum=0, rope_cs=True, rope_pos=False):
    """launch_gemm's routing for the forced families, restated (the module docstring names the line behind every False)"""
    if fam == "128":
        return True
    if dt != BF16 or b_km or accum:
        return False
    if epi == ROPE and (alpha != 1.0 or not rope_cs):
        return False
    if fam == "8p":
        return True
    if epi in (BIAS, GELU) or (epi == STORE and alpha != 1.0) or (epi == ROPE and (rope_pos or c_f32)):
        return False
    if fam == "8c":
        return True
    return epi in (RESID, ROPE, SWIGLU, SWIGLU_BWD) or (epi == STORE and not c_f32)


@pytest.fixture
def family(monkeypatch):
    """set(fam): the switches that force a family; the environment and the parsed switches are restored afterwards"""
    def set_family(fam):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in FAMILIES[fam][0].items():
            monkeypatch.setenv(k, v)
    yield set_family
    monkeypatch.undo()
    _lib().lib().rsys_switches_reload()


# ============================================================================================ cases and their fp64 references
def _pad8(n, extra):
    return (n + 7) // 8 * 8 + extra


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _sigmoid(a):
    return 1.0 / (1.0 + np.exp(-a))


def _erf(x):
    return np.vectorize(math.erf)(x)


def rope_tables(T, hd, exact, rng):
    """cos / sin [T][hd/2] as fp32.  True tables (precompute_freqs_cis of the reference model, theta = 500000), or the exact variant: row 0 =
    (1, 0), every other entry drawn from {0, +-1, +-0.5, +-0.25} with no (0, 0) and no identity (1, 0) pair"""
    if not exact:
        ang = np.outer(np.arange(T, dtype=np.float64), 1.0 / 500000.0 ** (np.arange(0, hd, 2, dtype=np.float64) / hd))
        return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    vals = np.array([0, 1, -1, 0.5, -0.5, 0.25, -0.25], np.float32)
    c = vals[rng.integers(0, 7, (T, hd // 2))]; s = vals[rng.integers(1, 7, (T, hd // 2))]   # s != 0: never (0, 0) nor the identity
    c[0] = 1.0; s[0] = 0.0
    return c, s


def make_case(epi, dt, M, N, K, integer, seed, c_f32=0, alpha=1.0, accum=0, rope=None):
    """Host arrays of one problem (storage-rounded), its fp64 reference and bounds.  rope = dict(T, hd, n_q, n_k, exact, explicit).
    Outputs: out["C"] / out["C2"] = (ref [M][w] f64, bound of the fp32 stage, T-typed?, exact?)."""
    rng = np.random.default_rng(seed)
    c = dict(epi=epi, dt=dt, M=M, N=N, K=K, integer=integer, c_f32=c_f32, alpha=alpha, accum=accum, rope=rope)
    if integer:
        A = rng.integers(-3, 4, (M, K)).astype(np.float32); B = rng.integers(-3, 4, (N, K)).astype(np.float32)
        A[0, :] = np.arange(K) % 5 - 2; B[:, 0] = np.arange(N) % 7 - 3
    else:
        A = storage(rng.standard_normal((M, K)), dt); B = storage(rng.standard_normal((N, K)), dt)
    A64 = A.astype(np.float64)
    lim = {SWIGLU: LIM, SWIGLU_BWD: LIM, GELU: LIM - 2.0}.get(epi)
    if lim is not None:   # a power-of-two scale of B keeps it representable and the integer accumulators exact
        mx = np.abs(A64 @ B.astype(np.float64).T).max()
        B = B * np.float32(2.0 ** -max(0, math.ceil(math.log2(mx / lim))))
    B64 = B.astype(np.float64)
    acc = A64 @ B64.T
    slack = np.zeros_like(acc) if integer else K * U * (np.abs(A64) @ np.abs(B64).T)
    c.update(A=A, B=B)

    def dy(lo, hi, q, shape):   # dyadic values k / q or fp32 normals
        return (rng.integers(lo * q, hi * q + 1, shape) / q).astype(np.float32) if integer else rng.standard_normal(shape).astype(np.float32)

    tdt = dt if not c_f32 else F32   # type of a "T or f32" C
    out = {}
    if epi == STORE:
        ref = alpha * acc; b = abs(alpha) * slack + U * np.abs(ref)          # alpha acc: 1 rounding
        if accum:
            c["prior"] = storage(dy(-8, 8, 2, (M, N)), tdt)
            ref = ref + c["prior"]; b = b + U * (np.abs(alpha * acc) + np.abs(c["prior"]))   # + C: 1 more
        out["C"] = (ref, b, not c_f32, integer)
    elif epi == ACCUM:
        c["prior"] = dy(-8, 8, 2, (M, N))
        out["C"] = (acc + c["prior"], slack + U * (np.abs(acc) + np.abs(c["prior"])), False, integer)
    elif epi == BIAS:
        c["bias"] = dy(-4, 4, 4, N)
        out["C"] = (acc + c["bias"], slack + U * (np.abs(acc) + np.abs(c["bias"])), not c_f32, integer)
    elif epi == RESID:
        c["resid"] = dy(-8, 8, 2, (M, N))
        out["C"] = (acc + c["resid"], slack + U * (np.abs(acc) + np.abs(c["resid"])), False, integer)
    elif epi == TABLE:
        c["bias"] = dy(-4, 4, 4, N); c["E"] = dy(-8, 8, 4, (M, N))
        ref = acc + c["E"].astype(np.float64) + c["bias"]                    # two additions: 2 roundings
        b = slack + 2 * U * (np.abs(acc) + np.abs(c["E"]) + np.abs(c["bias"]))
        out["C"] = (ref, b, False, integer); out["C2"] = (ref, b, True, integer)
    elif epi == GELU:
        c["bias"] = (dy(-2, 2, 4, N) if integer else np.clip(0.5 * rng.standard_normal(N), -2.0, 2.0)).astype(np.float32)
        z = acc + c["bias"]; ez = slack + U * (np.abs(acc) + np.abs(c["bias"]))
        assert np.abs(z).max() <= LIM
        er = _erf(z / math.sqrt(2.0)); phi = np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
        g = 0.5 * z * (1.0 + er)
        # t = z * fl(1 / sqrt 2): 2 roundings of the argument move erf by 2 |z| phi(z) * 2 U; erff: 2 ulp = 4 U |erf|; 1 + erf: U |1 + erf|;
        # 0.5 z is exact, the last product 1 rounding; d gelu / dz = (1 + erf) / 2 + z phi
        eg = np.abs(0.5 * z) * U * (4 * np.abs(z) * phi + 4 * np.abs(er) + np.abs(1.0 + er)) + U * np.abs(g) \
            + np.abs(0.5 * (1.0 + er) + z * phi) * ez
        out["C"] = (z, ez, True, integer); out["C2"] = (g, eg, True, False)
    elif epi == SWIGLU:
        assert N % 32 == 0 and np.abs(acc).max() <= LIM
        blk = acc.reshape(M, N // 32, 32); sl = slack.reshape(M, N // 32, 32)
        a, b_ = blk[:, :, :16], blk[:, :, 16:]; ea, eb = sl[:, :, :16], sl[:, :, 16:]
        s = _sigmoid(a); g = a * s * b_
        # sigmoid and the multiplies: relative (|a| + 8) U; dg/da = b s (1 + a (1 - s)), dg/db = a s
        eg = (np.abs(a) + 8) * U * np.abs(g) + np.abs(b_ * s * (1 + a * (1 - s))) * ea + np.abs(a * s) * eb
        out["C"] = (acc, slack, True, integer); out["C2"] = (g.reshape(M, N // 2), eg.reshape(M, N // 2), True, False)
    elif epi == SWIGLU_BWD:
        assert N % 16 == 0 and np.abs(acc).max() <= LIM
        ab = storage(dy(-8, 8, 4, (M, 2 * N)) if integer else rng.uniform(-LIM, LIM, (M, 2 * N)), dt)
        c["saved"] = ab
        blk = ab.astype(np.float64).reshape(M, N // 16, 32)
        a, b_ = blk[:, :, :16], blk[:, :, 16:]; dg = acc.reshape(M, N // 16, 16); edg = slack.reshape(M, N // 16, 16)
        s = _sigmoid(a); w = 1 + a * (1 - s)
        da = dg * b_ * s * w; db = dg * a * s
        es = (np.abs(a) + 8) * U                                              # relative error of s
        # es already counts the multiplies around s.  w = 1 + a (1 - s) is arithmetic of its own: 1 - s carries s es + U |1 - s|, the
        # product with a adds U |a (1 - s)|, the addition of 1 adds U |w|
        ew = np.abs(a) * (s * es + U * np.abs(1 - s)) + U * np.abs(a * (1 - s)) + U * np.abs(w)
        eda = np.abs(dg * b_ * s) * ew + np.abs(da) * es + np.abs(b_ * s * w) * edg
        edb = np.abs(db) * es + np.abs(a * s) * edg
        out["C"] = (np.concatenate([da, db], 2).reshape(M, 2 * N), np.concatenate([eda, edb], 2).reshape(M, 2 * N), True, False)
    elif epi == ROPE:
        T, hd, n_q, n_k = rope["T"], rope["hd"], rope["n_q"], rope["n_k"]
        cos, sin = rope_tables(T, hd, rope["exact"], rng)
        c.update(cos=cos, sin=sin, cs=np.stack([cos, sin], -1))
        if rope["explicit"]:   # non-monotonic, with repeats, 0 and T - 1 included
            pos = rng.integers(0, T, M).astype(np.int32)
            pos[1::3] = pos[0:-1:3][: len(pos[1::3])]
            pos[0] = T - 1; pos[M // 2] = 0; pos[M - 1] = T - 1
            c["pos"] = pos
        else:
            pos = np.arange(M) % T
        nqk = n_q + n_k
        col = np.arange(nqk); d = (np.where(col < n_q, col, col - n_q) % hd) // 2
        cm = cos.astype(np.float64)[pos][:, d[0::2]]; sm = sin.astype(np.float64)[pos][:, d[0::2]]
        v = alpha * acc; sv = abs(alpha) * slack                              # (alpha is a power of two: no rounding)
        v0, v1 = v[:, 0:nqk:2], v[:, 1:nqk:2]; s0, s1 = sv[:, 0:nqk:2], sv[:, 1:nqk:2]
        ref = v.copy(); b = sv.copy()                                         # the v columns: the identity
        ref[:, 0:nqk:2] = v0 * cm - v1 * sm; ref[:, 1:nqk:2] = v0 * sm + v1 * cm
        b[:, 0:nqk:2] = 3 * U * (np.abs(v0 * cm) + np.abs(v1 * sm)) + s0 * np.abs(cm) + s1 * np.abs(sm)
        b[:, 1:nqk:2] = 3 * U * (np.abs(v0 * sm) + np.abs(v1 * cm)) + s0 * np.abs(sm) + s1 * np.abs(cm)
        if accum:
            c["prior"] = storage(dy(-8, 8, 2, (M, N)), tdt)
            b = b + U * (np.abs(ref) + np.abs(c["prior"])); ref = ref + c["prior"]
        out["C"] = (ref, b, not c_f32, integer and rope["exact"])
    c["out"] = out
    c["slack_C"] = {STORE: abs(alpha) * slack, ROPE: None}.get(epi, slack)   # the part of C's bound that is accumulation-order slack
    if epi == ROPE:
        sl = sv.copy(); sl[:, 0:nqk:2] = s0 * np.abs(cm) + s1 * np.abs(sm); sl[:, 1:nqk:2] = s0 * np.abs(sm) + s1 * np.abs(cm)
        c["slack_C"] = sl
    return _freeze(c)


_CASES = {}


def case(*key, **kw):
    """make_case, computed once per key and shared (read-only) between the families of one epilogue"""
    k = (key, tuple(sorted((a, tuple(sorted(b.items())) if isinstance(b, dict) else b) for a, b in kw.items())))
    if k not in _CASES:
        if _CASES and next(iter(_CASES))[0][0] != key[0]:
            _CASES.clear()   # another epilogue: the earlier references are not needed again
        _CASES[k] = make_case(*key, **kw)
    return _CASES[k]


# ============================================================================================ launch and checks
def launch(dev, fam, c, b_km=0, m_dev=None, use_cs=True, refused=None):
    """one rsys_op_gemm_epi call; returns the whole C and C2 buffers ([M][ldc], [M][ldc2]) as fp32 values.  refused: the call must fail
    with that text in its error message and leave C as it was"""
    epi, dt, M, N, K = c["epi"], c["dt"], c["M"], c["N"], c["K"]
    wc = 2 * N if epi == SWIGLU_BWD else N                                   # logical widths of C and C2
    w2 = {SWIGLU: N // 2, TABLE: N, GELU: N, SWIGLU_BWD: 2 * N}.get(epi, 0)
    ldc = _pad8(wc, 8); ldc2 = ldc if epi == SWIGLU_BWD else _pad8(w2, 16); ldr = _pad8(N, 24)
    lda = _pad8(K, 8); ldb = _pad8(N if b_km else K, 8)
    As = np.zeros((M, lda), np.float32); As[:, :K] = c["A"]
    if b_km:
        Bs = np.zeros((K, ldb), np.float32); Bs[:, :N] = c["B"].T
    else:
        Bs = np.zeros((N, ldb), np.float32); Bs[:, :K] = c["B"]

    def padded(x, ld):
        full = np.full((M, ld), SENT, np.float32)
        if x is not None:
            full[:, : x.shape[1]] = x
        return full

    c_is_t = c["out"]["C"][2]
    cdt = dt if c_is_t else F32
    dA = dev.put(As, dt); dB = dev.put(Bs, dt)
    c_before = padded(c.get("prior"), ldc)
    dC = dev.put(c_before, cdt)
    dC2 = None
    if w2:
        dC2 = dev.put(padded(c.get("saved"), ldc2), dt)
    dbias = dev.put(c["bias"]) if "bias" in c else None
    dres = dev.put(padded(c["resid"], ldr)) if "resid" in c else None
    dE = dev.put(padded(c["E"], ldc)) if "E" in c else None
    dcos = dsin = dcs = dpos = None
    T = hd = n_q = n_k = 0
    if epi == ROPE:
        r = c["rope"]; T, hd, n_q, n_k = r["T"], r["hd"], r["n_q"], r["n_k"]
        dcos = dev.put(c["cos"]); dsin = dev.put(c["sin"])
        dcs = dev.put(c["cs"]) if use_cs else None
        dpos = dev.put(c["pos"]) if "pos" in c else None
    dm = dev.put(np.array([m_dev], np.int32)) if m_dev is not None else None
    tag = C.create_string_buffer(16); half = C.c_int32(-1)
    rc = dev.L.rsys_op_gemm_epi(dt, dA, dB, dC, M, N, K, lda, ldb, ldc, b_km, c["c_f32"], epi, C.c_float(c["alpha"]), c["accum"], dbias,
                                dres, ldr, dC2, ldc2, dE, dcos, dsin, dcs, dpos, T, hd, n_q, n_k, dm, tag, len(tag), C.byref(half))
    if refused is not None:
        assert rc != 0 and refused in _lib().last_error(), (rc, _lib().last_error())
        assert np.array_equal(dev.get(dC, (M, ldc), cdt), c_before), "a refused call wrote to C"
        dev.free()
        return None
    assert rc == 0, _lib().last_error()
    want = ("nn" if b_km else "nt") if fam == "128" else fam[:2]
    assert (tag.value.decode(), half.value) == (want, FAMILIES[fam][2]), (fam, EPI_NAMES[epi], tag.value, half.value)
    Cf = dev.get(dC, (M, ldc), cdt)
    C2f = dev.get(dC2, (M, ldc2), dt) if w2 else None
    dev.free()
    return Cf, C2f


RATIO = {}


def check(c, fam, got, name, rows=None, what=""):
    """got: the whole buffer of output `name`.  Rows [0, rows) against the reference (exact or bounded); every column >= the width untouched"""
    ref, bound, is_t, exact = c["out"][name]
    M, w = ref.shape
    rows = M if rows is None else rows
    assert np.all(got[:, w:] == SENT), f"{what} {name}: padding columns written"
    x = got[:rows, :w].astype(np.float64); ref = ref[:rows]; bound = bound[:rows]
    bf = is_t and c["dt"] == BF16
    if exact:
        want = bf16_round(ref) if bf else ref.astype(np.float32)
        bad = np.argwhere(x != want)
        assert bad.size == 0, f"{what} {name}: {len(bad)} elements differ, first (row, col) {bad[0]}: {x[tuple(bad[0])]} != {want[tuple(bad[0])]}"
        return
    tol = bound + (bf16_ulp(ref) if bf else 0.0)
    err = np.abs(x - ref)
    i = np.unravel_index(np.argmax(err - tol), err.shape) if err.size else None
    assert i is None or err[i] <= tol[i], f"{what} {name}: |{x[i]} - {ref[i]}| = {err[i]:.3e} > {tol[i]:.3e} at {i}"
    if err.size:
        r = float((err / np.maximum(tol, 1e-300)).max())
        key = (EPI_NAMES[c["epi"]], name, "bf16" if bf else "fp32")
        RATIO[key] = max(RATIO.get(key, 0.0), r)
        print(f"ratio {key[0]} {name} {key[2]} {fam}: max err / bound = {r:.3f} (worst so far {RATIO[key]:.3f}) {what}")


def run_and_check(dev, fam, c, b_km=0, what=""):
    Cf, C2f = launch(dev, fam, c, b_km)
    check(c, fam, Cf, "C", what=what)
    if "C2" in c["out"]:
        check(c, fam, C2f, "C2", what=what)
    return Cf, C2f


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ============================================================================================ every epilogue but RoPE, small shapes
# 256 family: one FULL tile at the shortest K; an edge tile in both directions (N % 8 == 0, the last 8-column group partly outside a
# 16-block, odd K-tile count); full tiles and a ragged last tile row (HALF: four full 128-row tiles and a ragged one).
# 128x128 kernel: one tile, ragged in both directions, smaller than a tile, and the LoRA K.
SHAPES = {"256": [(256, 256, 128), (300, 264, 192), (520, 512, 128)], "128": [(128, 128, 64), (200, 72, 104), (16, 40, 8), (64, 96, 16)]}
BIG = (16640, 512, 128)   # 130 tiles of 256 rows, 260 of 128 (HALF: more tiles than CUs, a workgroup goes on to a second tile)


def shape_for(epi, M, N, K):
    """the nearest N the epilogue takes: N % 32 == 0 for SwiGLU (264 -> 288, 72 -> 96), N % 16 == 0 for its backward (264 -> 272, 72 -> 80)"""
    q = {SWIGLU: 32, SWIGLU_BWD: 16}.get(epi, 8)
    return M, (N + q - 1) // q * q, K


# option sets per epilogue (c_f32, alpha, accum)
VARIANTS = {
    STORE: [dict(), dict(c_f32=1), dict(alpha=2.0), dict(c_f32=1, alpha=0.5), dict(accum=1), dict(accum=1, alpha=2.0)],
    ACCUM: [dict(c_f32=1)], BIAS: [dict(), dict(c_f32=1)], RESID: [dict(c_f32=1)], SWIGLU: [dict()], TABLE: [dict(c_f32=1)], GELU: [dict()],
    SWIGLU_BWD: [dict()],
}
EPI_FAM = [(e, cfg) for e in VARIANTS for cfg in CONFIGS if any(eligible(cfg[0], cfg[1], cfg[2], e, **v) for v in VARIANTS[e])]


@pytest.mark.parametrize("epi,cfg", EPI_FAM, ids=[f"{EPI_NAMES[e]}-{f}-{'bf16' if d else 'fp32'}-{'km' if k else 'rm'}" for e, (f, d, k) in EPI_FAM])
def test_epilogue(dev, family, epi, cfg):
    """Each epilogue on each family that has it, at the smallest shapes that reach every path (SHAPES), with integer / dyadic data (bit
    exact) and with random data (derived bounds).  gemm8c's HALF form must agree with its full form bit for bit."""
    fam, dt, b_km = cfg
    ran = 0
    for (M, N, K) in SHAPES["128" if fam == "128" else "256"]:
        M, N, K = shape_for(epi, M, N, K)
        for v in VARIANTS[epi]:
            if not eligible(fam, dt, b_km, epi, **v):
                continue
            for integer in (True, False):
                c = case(epi, dt, M, N, K, integer, 1000 * epi + M + N + K, **v)
                family(fam)
                what = f"{fam} {M}x{N}x{K} {v} {'int' if integer else 'rnd'}"
                got = run_and_check(dev, fam, c, b_km, what)
                ran += 1
                if fam == "8ch":
                    family("8c")
                    full = launch(dev, "8c", c)
                    for g, f in zip(got, full):
                        assert (g is None and f is None) or np.array_equal(bits(g), bits(f)), f"HALF != full form: {what}"
    assert ran > 0


@pytest.mark.parametrize("epi", [RESID, ACCUM, TABLE, SWIGLU_BWD])
def test_epilogue_many_tiles(dev, family, epi):
    """The epilogues that read an operand, on 130 (HALF: 260) row tiles: in the HALF form a workgroup finishes one tile's epilogue while it
    starts the next tile.  The hand-over depends on timing: two runs must agree bit for bit, and the forms of gemm8c with each other."""
    M, N, K = BIG
    for integer in ((False,) if epi == SWIGLU_BWD else (True, False)):   # (nothing of the SwiGLU backward is exact)
        c = make_case(epi, BF16, M, N, K, integer, 77 + epi, **VARIANTS[epi][0])
        outs = {}
        for fam in FAM256:
            if not eligible(fam, BF16, 0, epi, **VARIANTS[epi][0]):
                continue
            family(fam)
            first = run_and_check(dev, fam, c, what=f"{fam} big {'int' if integer else 'rnd'}")
            second = launch(dev, fam, c)
            for a, b in zip(first, second):
                assert (a is None and b is None) or np.array_equal(bits(a), bits(b)), f"{fam}: two runs differ"
            outs[fam] = first
        if "8ch" in outs:
            for a, b in zip(outs["8c"], outs["8ch"]):
                assert (a is None and b is None) or np.array_equal(bits(a), bits(b)), "HALF != full form"


# ============================================================================================ QKV + RoPE
LAYOUTS = [(4, 1, 16), (2, 1, 64), (2, 2, 128)]   # (H, KV, hd): N = 96 (q/k and k/v boundaries inside one wave's 64 columns), 256, 768 (a head spans two wave blocks)
ROPE_T = [48, 96, 128, 136]                      # % T branch (48, 96), single-subtract branch (128, 136); 136: a 16-row block wraps mid-block


def rope_opts(H, KV, hd, T, exact, explicit=False):
    return dict(T=T, hd=hd, n_q=H * hd, n_k=KV * hd, exact=exact, explicit=explicit)


ROPE_CFG = [(cfg, lay) for cfg in CONFIGS for lay in LAYOUTS]


@pytest.mark.parametrize("cfg,lay", ROPE_CFG, ids=[f"{f}-{'bf16' if d else 'fp32'}-{'km' if k else 'rm'}-H{h}KV{kv}hd{hd}" for (f, d, k), (h, kv, hd) in ROPE_CFG])
def test_rope(dev, family, cfg, lay):
    """EPI_QKV_ROPE with implicit positions row % T: every T branch, M a multiple of T (256 = 2 x 128; 128 x 128 kernel: 128) and not, exact
    dyadic tables (bit equality) and true tables (3 roundings); explicit positions and fp32 C where the family has them."""
    fam, dt, b_km = cfg
    H, KV, hd = lay
    N = (H + 2 * KV) * hd
    for (M, _, K) in SHAPES["128" if fam == "128" else "256"]:
        for T in ROPE_T:
            for exact in (True, False):
                opts = [dict(), dict(c_f32=1)] + ([dict(explicit=True), dict(explicit=True, c_f32=1)] if T == 136 else [])
                for o in opts:
                    explicit = o.get("explicit", False); c_f32 = o.get("c_f32", 0)
                    if not eligible(fam, dt, b_km, ROPE, c_f32=c_f32, rope_pos=explicit):
                        continue
                    c = case(ROPE, dt, M, N, K, exact, 5000 + M + N + K + T, c_f32=c_f32, rope=rope_opts(H, KV, hd, T, exact, explicit))
                    family(fam)
                    what = f"{fam} {M}x{N}x{K} T={T} {'exact' if exact else 'true'} {o}"
                    got = run_and_check(dev, fam, c, b_km, what)
                    if fam == "8ch":
                        family("8c")
                        assert np.array_equal(bits(got[0]), bits(launch(dev, "8c", c)[0])), f"HALF != full form: {what}"


def test_rope_many_tiles(dev, family):
    """RoPE at (16640, 512, 128), heads (4, 2, 64): 130 tiles of 256 rows, 260 of 128 in the HALF form -- more than the CUs, so a workgroup
    finishes one tile's RoPE epilogue (prefetched table rows, pending stores) while it starts its next tile, whose row % T starts
    anew.  T = 136 (16640 is no multiple of it), exact tables: bit equal to the reference, two runs bit equal, and the two forms of
    gemm8c with each other"""
    M, N, K = BIG
    H, KV, hd = 4, 2, 64
    assert (H + 2 * KV) * hd == N
    c = make_case(ROPE, BF16, M, N, K, True, 91, rope=rope_opts(H, KV, hd, 136, True))
    outs = {}
    for fam in FAM256:
        family(fam)
        outs[fam] = run_and_check(dev, fam, c, what=f"{fam} big")[0]
        assert np.array_equal(bits(outs[fam]), bits(launch(dev, fam, c)[0])), f"{fam}: two runs differ"
    assert np.array_equal(bits(outs["8c"]), bits(outs["8ch"])), "HALF != full form"


@pytest.mark.parametrize("dt", [F32, BF16])
def test_rope_without_interleaved_table_and_lora_form(dev, family, dt):
    """Without rope_cs the product runs on the 128x128 kernel even when the 256 family is forced (asserted: tag "nt"), from the two plain
    tables.  The LoRA form: K = 16, alpha = 2, accum = 1 into a T-typed C of dyadic values (128x128 kernel, both dtypes), for RoPE and for
    a plain store."""
    H, KV, hd = 2, 1, 64
    N = (H + 2 * KV) * hd
    for exact in (True, False):
        c = case(ROPE, dt, 300, N, 192, exact, 17, rope=rope_opts(H, KV, hd, 96, exact))
        family("8p")   # forced, but not eligible without the interleaved table
        Cf, _ = launch(dev, "128", c, use_cs=False)
        check(c, "128", Cf, "C", what="no rope_cs")
        for (M, K) in [(64, 16), (200, 16)]:
            family("128")
            c = case(ROPE, dt, M, N, K, exact, 23 + M, alpha=2.0, accum=1, rope=rope_opts(H, KV, hd, 48, exact))
            run_and_check(dev, "128", c, what=f"lora rope {M} {'exact' if exact else 'true'}")
            c = case(STORE, dt, M, 96, K, exact, 29 + M, alpha=2.0, accum=1)
            run_and_check(dev, "128", c, what=f"lora store {M}")


def test_rope_rejects_regions_that_are_not_whole_heads(dev, family):
    """epi_item rotates items of 8 consecutive columns as one head's pairs: a q or k region that is not a whole number of heads would put
    an item across the boundary.  launch_gemm refuses such a problem (and a region past N, and T = 0 without positions) before anything
    is launched: the call fails with that message and C, read back, still holds its sentinel everywhere."""
    H, KV, hd = 2, 1, 64
    N = (H + 2 * KV) * hd
    good = make_case(ROPE, BF16, 64, N, 16, True, 3, rope=rope_opts(H, KV, hd, 48, True))
    family("128")
    run_and_check(dev, "128", good)
    for bad in (dict(n_q=H * hd - 4), dict(n_k=KV * hd + 4), dict(n_k=KV * hd + 8), dict(n_q=N, n_k=hd), dict(T=0)):
        c = dict(good); c["rope"] = {**good["rope"], **bad}
        assert launch(dev, "128", c, refused="rope epilogue needs") is None


# ============================================================================================ device-side row count
MDEV_EPI = [RESID, SWIGLU, SWIGLU_BWD, GELU, STORE]
MDEV_CFG = [(e, cfg) for e in MDEV_EPI for cfg in [("128", F32, 0), ("128", BF16, 0), ("8p", BF16, 0), ("8c", BF16, 0), ("8ch", BF16, 0)]
            if eligible(cfg[0], cfg[1], cfg[2], e)]


@pytest.mark.parametrize("epi,cfg", MDEV_CFG, ids=[f"{EPI_NAMES[e]}-{f}-{'bf16' if d else 'fp32'}" for e, (f, d, k) in MDEV_CFG])
def test_device_side_row_count(dev, family, epi, cfg):
    """m_dev in {0, 1, 257, M}: rows below *m_dev are correct (bit exact on integer data), rows from the end of the last started tile on
    (128 rows per tile; 256 in gemm8p and gemm8c's full form) still hold the sentinel -- the contract rsys_op_gemm_rows documents"""
    fam, dt, b_km = cfg
    tile = FAMILIES[fam][1]
    M, N, K = shape_for(epi, *((520, 72, 104) if fam == "128" else (520, 512, 128)))
    v = VARIANTS[epi][0]
    for integer in (True, False):
        c = case(epi, dt, M, N, K, integer, 300 + epi, **v)
        for m in (0, 1, 257, M):
            family(fam)
            Cf, C2f = launch(dev, fam, c, b_km, m_dev=m)
            end = min(M, (m + tile - 1) // tile * tile)
            for name, got in (("C", Cf), ("C2", C2f)):
                if name not in c["out"]:
                    continue
                check(c, fam, got, name, rows=m, what=f"{fam} m_dev={m}")
                w = c["out"][name][0].shape[1]
                keep = c["saved"] if (name == "C2" and epi == SWIGLU_BWD) else None   # (C2 is an input there: never written)
                assert np.all(got[end:, :w] == (SENT if keep is None else keep[end:])), f"{fam} {name} m_dev={m}: rows >= {end} written"
                if keep is not None:
                    assert np.array_equal(got[:, :w], keep)


# ============================================================================================ families against each other
CROSS = [(STORE, dict(c_f32=1)), (ACCUM, dict(c_f32=1)), (BIAS, dict(c_f32=1)), (RESID, dict(c_f32=1)), (TABLE, dict(c_f32=1)), (ROPE, dict(c_f32=1))]


@pytest.mark.parametrize("epi,v", CROSS, ids=[EPI_NAMES[e] for e, _ in CROSS])
def test_families_agree_on_fp32_outputs(dev, family, epi, v):
    """Random operands, fp32 outputs, ragged shapes: the families add the same K products in different orders, then apply the same
    epilogue.  Two results agree within the accumulation-order slack K U sum|a b| (propagated through the epilogue) plus the epilogue's
    counted roundings once per side."""
    for (M, N, K) in SHAPES["256"][1:]:
        if epi == ROPE:
            N = 256; v = dict(c_f32=1, rope=rope_opts(2, 1, 64, 136, False))
        c = case(epi, BF16, M, N, K, False, 40 + epi + M, **v)
        bound = c["out"]["C"][1]; slack = c["slack_C"]
        tol = slack + 2 * (bound - slack)
        outs = {}
        for fam in ("128",) + FAM256:
            if eligible(fam, BF16, 0, epi, c_f32=1):
                family(fam)
                outs[fam] = launch(dev, fam, c)[0][:, :N].astype(np.float64)
        assert len(outs) >= 2
        names = list(outs)
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                err = np.abs(outs[a] - outs[b])
                j = np.unravel_index(np.argmax(err - tol), err.shape)
                assert err[j] <= tol[j], f"{EPI_NAMES[epi]} {a} vs {b}: {err[j]:.3e} > {tol[j]:.3e} at {j}"
                print(f"cross {EPI_NAMES[epi]} {a} vs {b} {M}x{N}x{K}: max diff / tol = {(err / np.maximum(tol, 1e-300)).max():.3f}")
