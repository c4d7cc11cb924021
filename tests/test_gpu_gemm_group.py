"""GPU: the grouped weight-gradient launch (csrc/gemm8p.hip: gemm8p_group_plan_create + launch_gemm8p_group) and the fp8 split-K product
(launch_gemm8p_f8_splitk), alone, through rsys_op_gemm_group / rsys_op_gemm_f8_splitk (rsys_debug.h): every arm -- gemm4k_group_kernel,
gemm8p_group_kernel, the ordered (slab) form and gemm8p_group_f8_kernel -- against A^T B in float64 from the same operand values.

The exact cases use small integers (|a|, |b| <= 3, K <= 2048, at most two launches: every partial sum stays below 2^24, so bf16, fp8 and fp32
hold everything exactly and no summation order can matter) with one asymmetric row and column, power-of-two fp8 descales, and ONE gradient
buffer for all products of a plan: non-zero integers C0 everywhere, the products' C back to back with ldc = N + 8 or N and small gaps, a
guard region at both ends.  The whole buffer is compared with assert_array_equal: the products' columns hold C0 + launches * ref, the
padding columns, the gaps and the guards still hold C0.  K-major bf16 operands are followed by 64 rows of +-1e30 and padded with non-zero
columns; fp8 rows are padded with the formats' largest codes: a read past K or past M / N that reaches a sum shows."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K8G, K4KG, K8GF = 0, 1, 2          # RSYS_GROUP_KERNEL_* (rsys_debug.h)
ERR_ARG = -1
# (name, RSYS_GEMM4K, ordered, the kernel the hook must report)
ARMS = [("4kg", "1", False, K4KG), ("8g", "0", False, K8G), ("ordered", None, True, K8G)]
ARM_IDS = [a[0] for a in ARMS]


def _lib():
    from recommendersystem_amd import _lib
    return _lib.lib(), _lib


def _bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + 0x7FFF
    return ((u + r) & 0xFFFF0000).view(np.float32)


def _pack(x):
    return (_bf16_round(x).view(np.uint32) >> 16).astype(np.uint16)


def _dev(lib, arr):
    arr = np.ascontiguousarray(arr)
    p = C.c_void_p()
    assert lib.rsys_dev_alloc(C.byref(p), max(arr.nbytes, 64)) == 0
    assert lib.rsys_dev_h2d(p, arr.ctypes.data, arr.nbytes) == 0
    return p


def _set_arm(monkeypatch, arm, force):
    name, g4k, ordered, kernel = arm
    if g4k is None: monkeypatch.delenv("RSYS_GEMM4K", raising=False)
    else: monkeypatch.setenv("RSYS_GEMM4K", g4k)
    if force is None: monkeypatch.delenv("RSYS_DEBUG_8G_SPLITK", raising=False)
    else: monkeypatch.setenv("RSYS_DEBUG_8G_SPLITK", str(force))
    return ordered, kernel


# ---------------------------------------------------------------- products
class Prod:
    """one product C[M][N] += A^T B.  bf16: A (K, M), B (K, N) values, K-major storage.  fp8: A (M, K) e5m2, B (N, K) e4m3 values, K-contiguous
    storage, desc = the 32 descale floats.  ref = the float64 sum per launch as it lands in C (descaled, rows mapped)."""

    def __init__(self, A, B, f8=0, desc=None, rseg=0, rowmode=0, wide=False):
        self.A, self.B, self.f8, self.rseg, self.rowmode = A, B, f8, rseg, rowmode
        if f8:
            (self.M, self.K), self.N = A.shape, B.shape[0]
            self.lda = self.K + (16 if wide else 0); self.ldb = self.K + (0 if wide else 32)
            self.desc = np.zeros(32, np.float32); self.desc[:len(desc)] = desc
            r = np.arange(self.M)
            ref = (A.astype(np.float64) @ B.astype(np.float64).T) * self.desc[r // rseg if rseg else 0 * r].astype(np.float64)[:, None]
            if rowmode == 1:
                isb = (r >= self.M // 2).astype(int); i = r - isb * (self.M // 2)
                orow = (i >> 4) * 32 + isb * 16 + (i & 15)
                assert sorted(orow) == list(r)
                mapped = np.zeros_like(ref); mapped[orow] = ref; ref = mapped
            self.ref = ref
        else:
            (self.K, self.M), self.N = A.shape, B.shape[1]
            self.lda = self.M + (8 if wide else 0); self.ldb = self.N + (0 if wide else 8)
            self.desc = None
            self.ref = A.astype(np.float64).T @ B.astype(np.float64)

    def storage(self):
        """(A bytes, B bytes) as the kernels read them"""
        if self.f8:
            from oracle import fp8
            out = []
            for v, ld, fmt, poison in ((self.A, self.lda, fp8.E5M2, 0x7B), (self.B, self.ldb, fp8.E4M3, 0x7E)):   # 57344 / 448: the largest finite codes
                codes = fp8.encode_fp8(v, fmt)
                assert np.array_equal(fp8.decode_fp8(codes, fmt), v.astype(np.float32))
                s = np.full((v.shape[0], ld), poison, np.uint8); s[:, :self.K] = codes
                out.append(s.tobytes() + bytes([poison]) * 4096)
            return out
        out = []
        for v, ld, poison in ((self.A, self.lda, 1e30), (self.B, self.ldb, -1e30)):
            s = np.full((self.K + 64, ld), poison, np.float32)
            s[:self.K] = 7.0; s[:self.K, :v.shape[1]] = v          # padding columns: finite, non-zero, never part of a sum
            assert np.array_equal(_bf16_round(v), v)
            out.append(_pack(s).tobytes())
        return out


def _ints(rng, shape):
    return rng.integers(-3, 4, shape).astype(np.float32)


def int_prod(M, N, K, seed):
    rng = np.random.default_rng([M, N, K, seed])
    A, B = _ints(rng, (K, M)), _ints(rng, (K, N))
    A[:, 0] = np.arange(K) % 5 - 2; B[0, :] = np.arange(N) % 7 - 3
    return Prod(A, B, wide=bool(seed & 1))


def normal_prod(M, N, K, seed):
    rng = np.random.default_rng([M, N, K, seed, 77])
    return Prod(_bf16_round(rng.standard_normal((K, M))), _bf16_round(rng.standard_normal((K, N))), wide=bool(seed & 1))


def f8_prod(M, N, K, seed, desc=(1.0,), rseg=0, rowmode=0):
    rng = np.random.default_rng([M, N, K, seed, 8])
    A, B = _ints(rng, (M, K)), _ints(rng, (N, K))
    A[0, :] = np.arange(K) % 5 - 2; B[:, 0] = np.arange(N) % 7 - 3
    A[:, 1] = np.arange(M) % 7 - 3                                  # every output row its own data
    return Prod(A, B, f8=2, desc=desc, rseg=rseg, rowmode=rowmode, wide=bool(seed & 1))


# tiles 256 x 256, bf16 K tiles of 64: one partial tile and one K tile | a ragged second tile row, 7 K tiles | K tail of 40 | 4 x 3 tiles, both edges
# ragged, K tail | 10 tile columns (no band remap in the grouped form) | 3 K tiles with a tail of 1
MIXED = [(8, 8, 64), (264, 72, 448), (512, 256, 1000), (776, 520, 1536 - 24), (256, 2312, 200), (1408, 512, 129)]


@functools.lru_cache(maxsize=None)
def mixed_prods():
    return tuple(int_prod(M, N, K, i) for i, (M, N, K) in enumerate(MIXED))


@functools.lru_cache(maxsize=None)
def small_prods(n):
    """8 x 8 x 64 to 72 x 40 x 200, every product its own data"""
    Ks = (64, 200, 72, 129, 136)
    return tuple(int_prod(8 + 8 * (i % 9), 8 + 8 * (i % 5), Ks[i % 5], 1000 + i) for i in range(n))


# ---------------------------------------------------------------- one call
class Call:
    """the device side of one plan: operands and descales packed into one allocation, ONE gradient buffer [guard | C_0 | gap | C_1 | ... | guard]"""
    GUARD = 4096

    def __init__(self, prods, c0="ints", ldc_of=None):
        self.lib, self.L = _lib()
        self.prods = prods
        blobs, self.a_off, self.b_off, self.d_off = bytearray(), [], [], []
        def put(b):
            at = len(blobs); blobs.extend(b); blobs.extend(bytes(-len(blobs) % 256)); return at
        for p in prods:
            a, b = p.storage()
            self.a_off.append(put(a)); self.b_off.append(put(b))
            self.d_off.append(put(p.desc.tobytes()) if p.f8 else None)
        self.ldc, self.c_off = [], []
        at = self.GUARD
        for i, p in enumerate(prods):
            ldc = ldc_of(i, p) if ldc_of else p.N + (8 if i % 2 == 0 else 0)
            self.ldc.append(ldc); self.c_off.append(at)
            at += p.M * ldc + (0, 8, 4)[i % 3]                       # (gaps keep every C 16-byte aligned: the ordered sum's float4)
        self.total = at + self.GUARD
        rng = np.random.default_rng(len(prods) + self.total)
        if c0 == "ints":
            self.C0 = rng.integers(1, 6, self.total).astype(np.float32) * rng.choice(np.array([-1.0, 1.0], np.float32), self.total)
        else:
            self.C0 = np.zeros(self.total, np.float32)
        self.d_ops = _dev(self.lib, np.frombuffer(bytes(blobs), np.uint8))
        self.d_C = _dev(self.lib, self.C0)

    def close(self):
        self.lib.rsys_dev_free(self.d_ops); self.lib.rsys_dev_free(self.d_C)

    def view(self, buf, i):
        p = self.prods[i]
        return buf[self.c_off[i]:self.c_off[i] + p.M * self.ldc[i]].reshape(p.M, self.ldc[i])

    def expected(self, launches):
        want = self.C0.astype(np.float64)
        for i, p in enumerate(self.prods):
            self.view(want, i)[:, :p.N] += launches * p.ref
        return want

    def read(self):
        out = np.empty(self.total, np.float32)
        assert self.lib.rsys_dev_d2h(out.ctypes.data, self.d_C, out.nbytes) == 0
        return out

    def group(self, ordered=False, launches=1, n=None):
        """rsys_op_gemm_group on all products, or on n of them taken round-robin (refused plans only) -> (rc, split count, kernel)"""
        ps = self.prods if n is None else [self.prods[i % len(self.prods)] for i in range(n)]
        idx = list(range(len(self.prods))) if n is None else [i % len(self.prods) for i in range(n)]
        n = len(ps)
        ops = self.d_ops.value
        vp = lambda vals: (C.c_void_p * n)(*vals)
        i32 = lambda vals: (C.c_int32 * n)(*vals)
        i64 = lambda vals: (C.c_int64 * n)(*vals)
        sk, kern = C.c_int32(-1), C.c_int32(-1)
        rc = self.lib.rsys_op_gemm_group(
            n, vp([ops + self.a_off[i] for i in idx]), vp([ops + self.b_off[i] for i in idx]), vp([self.d_C.value + 4 * self.c_off[i] for i in idx]),
            i32([p.M for p in ps]), i32([p.N for p in ps]), i32([p.K for p in ps]), i64([p.lda for p in ps]), i64([p.ldb for p in ps]),
            i64([self.ldc[i] for i in idx]), i32([p.f8 for p in ps]),
            vp([ops + self.d_off[i] if self.d_off[i] is not None else None for i in idx]), i32([p.rseg for p in ps]), i32([p.rowmode for p in ps]),
            int(ordered), launches, C.byref(sk), C.byref(kern))
        return rc, sk.value, kern.value

    def f8_single(self, i, launches=1):
        p = self.prods[i]
        ops = self.d_ops.value
        return self.lib.rsys_op_gemm_f8_splitk(ops + self.a_off[i], ops + self.b_off[i], self.d_C.value + 4 * self.c_off[i], p.M, p.N, p.K, p.lda, p.ldb,
                                               self.ldc[i], ops + self.d_off[i], p.rseg, p.rowmode, launches)

    def check_exact(self, launches, what=""):
        out, want = self.read(), self.expected(launches)
        assert np.abs(want).max() < 2 ** 24
        for i, p in enumerate(self.prods):                          # per product first: the message names the product
            got, w = self.view(out, i), self.view(want, i)
            np.testing.assert_array_equal(got[:, :p.N], w[:, :p.N].astype(np.float32), err_msg=f"{what} product {i}: {p.M} x {p.N} x {p.K}")
            np.testing.assert_array_equal(got[:, p.N:], w[:, p.N:].astype(np.float32), err_msg=f"{what} product {i}: padding columns")
        np.testing.assert_array_equal(out[:self.GUARD], self.C0[:self.GUARD], err_msg=f"{what} front guard")
        np.testing.assert_array_equal(out[-self.GUARD:], self.C0[-self.GUARD:], err_msg=f"{what} guard behind the last product")
        np.testing.assert_array_equal(out, want.astype(np.float32), err_msg=f"{what} gaps between the products")


def run_exact(prods, ordered, kernel, launches=1, force=None):
    c = Call(prods)
    try:
        rc, sk, kern = c.group(ordered, launches)
        assert rc == 0, c.L.last_error()
        assert kern == kernel, (kern, kernel)
        if force is None: assert 1 <= sk <= 16, sk
        else: assert sk == force, (sk, force)
        c.check_exact(launches, f"split {sk} kernel {kern} ordered {ordered}")
    finally:
        c.close()
    return sk


# ---------------------------------------------------------------- bf16 arms, exact
@pytest.mark.parametrize("force", [None, 1, 2, 5, 16])
@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
def test_group_products_of_different_shapes_one_plan(monkeypatch, arm, force):
    """Six products of different M, N and K in one plan (MIXED), the split count left to the plan or forced: with 5 splits the 7-K-tile product has
    per = 2 and no work in split 4, with 5 or 16 the 1-K-tile product works in split 0 only (the ordered form reads those slabs back as cleared);
    the last split of every product ends at K, inside a K tile."""
    ordered, kernel = _set_arm(monkeypatch, arm, force)
    run_exact(mixed_prods(), ordered, kernel, force=force)


@pytest.mark.parametrize("n,force", [(1, None), (8, None), (9, None), (37, None), (128, None), (9, 3), (128, 3)])
@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
def test_group_product_counts(monkeypatch, arm, n, force):
    """1 to 128 small products with distinct data: a wrong product index in the work word (product << 24 | split << 16 | tile) shows as a wrong block;
    up to 8 products leave XCD lists empty (the early return), more put several products into one list.  Forced to 3 splits the 4-K-tile products have
    per = 2: split 2 has no work, and the products of 1 to 3 K tiles stop earlier."""
    ordered, kernel = _set_arm(monkeypatch, arm, force)
    run_exact(small_prods(n), ordered, kernel, force=force)


@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
def test_group_plan_launched_twice(monkeypatch, arm):
    """one plan, two launches: C0 + 2 ref.  The ordered form must clear its slabs per launch."""
    ordered, kernel = _set_arm(monkeypatch, arm, 5)
    run_exact(mixed_prods(), ordered, kernel, launches=2, force=5)


def test_ordered_splits_without_work_read_back_as_cleared(monkeypatch):
    """The ordered form's slabs [split][M][N] come from the allocator as they are; the (product, split) pairs without work are never written by the
    product kernel, so the launch's clear is all that stands between them and the sum.  An allocation of the slabs' size is filled with 0x7F bytes
    (3.4e38 as floats) and freed right before the call, so that a slab that reuses it starts dirty."""
    ordered, kernel = _set_arm(monkeypatch, ARMS[2], 5)
    prods = mixed_prods()[:2] + small_prods(3)
    lib, _ = _lib()
    slab_bytes = 5 * sum(p.M * p.N for p in prods) * 4
    for _ in range(2):
        dirty = C.c_void_p()
        assert lib.rsys_dev_alloc(C.byref(dirty), slab_bytes) == 0
        assert lib.rsys_dev_memset(dirty, 0x7F, slab_bytes) == 0
        assert lib.rsys_dev_free(dirty) == 0
        run_exact(prods, ordered, kernel, launches=2, force=5)


# ---------------------------------------------------------------- bf16 arms, random data
def _run_normal(prods, ordered, kernel, force):
    c = Call(prods, c0="zeros")
    try:
        rc, sk, kern = c.group(ordered)
        assert rc == 0, c.L.last_error()
        assert (sk, kern) == (force, kernel)
        out = c.read()
        return [c.view(out, i)[:, :p.N].copy() for i, p in enumerate(prods)]
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def twelve_normal():
    """twelve products of random normal bf16 operands; [4] is the one the tests look at (16 K tiles less a tail, 3 x 2 ragged tiles)"""
    shapes = [(72, 40, 200), (264, 72, 448), (8, 8, 64), (512, 256, 1000), (520, 264, 1000), (256, 264, 129), (40, 24, 136), (776, 520, 512), (16, 8, 72),
              (264, 256, 320), (64, 72, 64), (1408, 512, 129)]
    return tuple(normal_prod(M, N, K, i) for i, (M, N, K) in enumerate(shapes))


def test_ordered_form_is_reproducible_and_independent_of_neighbours(monkeypatch):
    """The ordered form at 4 splits on random data: (a) two runs agree bit for bit; (b) a product's result is the same bits whether it is alone in a plan or
    the 5th of 12 (the sum depends neither on scheduling nor on neighbours); (c) within 1e-5 max|ref| of float64, test_gemm_kmajor_lds_dma_kernel's bound
    for these kernels."""
    ordered, kernel = _set_arm(monkeypatch, ARMS[2], 4)
    prods = twelve_normal()
    run1 = _run_normal(prods, ordered, kernel, 4)
    run2 = _run_normal(prods, ordered, kernel, 4)
    for i, (a, b) in enumerate(zip(run1, run2)):
        np.testing.assert_array_equal(a, b, err_msg=f"two runs, product {i}")
    alone = _run_normal((prods[4],), ordered, kernel, 4)[0]
    np.testing.assert_array_equal(alone, run1[4], err_msg="alone against 5th of 12")
    for i, p in enumerate(prods):
        err = np.abs(run1[i] - p.ref).max() / np.abs(p.ref).max()
        print(f"ordered product {i} {p.M} x {p.N} x {p.K}: rel err {err:.3e}")
        assert err < 1e-5, (i, err)


@pytest.mark.parametrize("arm", ARMS[:2], ids=ARM_IDS[:2])
def test_atomic_arms_one_split_match_the_product_alone(monkeypatch, arm):
    """One K split: one atomic add per element, so a product's result in the group is the same bits as the product alone, and within 1e-5 max|ref| of
    float64 on random data."""
    ordered, kernel = _set_arm(monkeypatch, arm, 1)
    prods = twelve_normal()
    group = _run_normal(prods, ordered, kernel, 1)
    for i in (4, 7, 11):
        alone = _run_normal((prods[i],), ordered, kernel, 1)[0]
        np.testing.assert_array_equal(alone, group[i], err_msg=f"product {i}")
    for i, p in enumerate(prods):
        err = np.abs(group[i] - p.ref).max() / np.abs(p.ref).max()
        print(f"{arm[0]} product {i} {p.M} x {p.N} x {p.K}: rel err {err:.3e}")
        assert err < 1e-5, (i, err)


# ---------------------------------------------------------------- fp8
F8_CASES = {
    "plain-72x64x256": dict(M=72, N=64, K=256, desc=(0.25,)),
    "plain-520x264x1152": dict(M=520, N=264, K=1152, desc=(2.0,)),
    # rows 95|96, 191|192, 287|288 inside tiles, segment 2 across the 256-row tile edge
    "rseg-384-96": dict(M=384, N=72, K=256, desc=(0.5, 4.0, 0.125, 2.0), rseg=96),
    "rseg-200-13": dict(M=200, N=72, K=256, desc=tuple(2.0 ** (e % 7 - 3) for e in range(16)), rseg=13),     # 16 segments: the most
    # W13's row map, one 32-row block per half | three row tiles, the halves meet inside the second
    "rowmode-64": dict(M=64, N=40, K=256, desc=(0.5, 2.0), rseg=32, rowmode=1),
    "rowmode-608": dict(M=608, N=264, K=384, desc=(4.0, 0.25), rseg=304, rowmode=1),
}


@pytest.mark.parametrize("case", list(F8_CASES), ids=list(F8_CASES))
def test_f8_splitk_product_alone_and_in_a_plan(monkeypatch, case):
    """e5m2 dY8^T [M][K] times e4m3 X8^T [N][K] with the row descales f8_desc[row / f8_rseg] and W13's row map f8_rowmode == 1, exact: once through
    launch_gemm8p_f8_splitk (its own split count; two launches onto non-zero C0) and once as the only product of a grouped plan (gemm8p_group_f8_kernel)."""
    _set_arm(monkeypatch, ARMS[0], None)
    p = f8_prod(seed=len(case), **F8_CASES[case])
    for how in ("single", "group"):
        c = Call((p,))
        try:
            if how == "single":
                assert c.f8_single(0, launches=2) == 0, c.L.last_error()
            else:
                rc, sk, kern = c.group(launches=2)
                assert rc == 0, c.L.last_error()
                assert kern == K8GF and 1 <= sk <= 16, (kern, sk)
            c.check_exact(2, f"{case} {how}")
        finally:
            c.close()


def test_f8_seventeen_row_segments_are_refused():
    """M = 200 with f8_rseg = 12 is 17 descale segments, one more than f8_desc holds: both launchers refuse, nothing runs"""
    p = f8_prod(200, 72, 256, 3, desc=(1.0,) * 16, rseg=12)
    c = Call((p,))
    try:
        assert c.f8_single(0) == ERR_ARG
        assert "fp8 split-K GEMM" in c.L.last_error(), c.L.last_error()
        rc, _, _ = c.group()
        assert rc == ERR_ARG
        assert "grouped GEMM" in c.L.last_error(), c.L.last_error()
        np.testing.assert_array_equal(c.read(), c.C0)
    finally:
        c.close()


def test_f8_group_two_layers_three_splits(monkeypatch):
    """The four weight-gradient products of f8_dw_params (w2, w13, wo, wqkv, in that order) for two small layers, each with its own block of descales, in
    one plan forced to 3 splits with K = 640: 5 K tiles of 128, per = 2, the last split is short.  Two launches onto non-zero C0."""
    _set_arm(monkeypatch, ARMS[0], 3)
    prods, K = [], 640
    for l, (D, Ip, Nqkv, kvhd) in enumerate([(64, 48, 64, 16), (264, 272, 320, 80)]):
        d = lambda j, k: tuple(2.0 ** ((l * 5 + j * 3 + e) % 6 - 3) for e in range(k))
        prods += [f8_prod(D, Ip, K, 10 * l, desc=d(0, 1)),
                  f8_prod(2 * Ip, D, K, 10 * l + 1, desc=d(1, 2), rseg=Ip, rowmode=1),
                  f8_prod(D, D, K, 10 * l + 2, desc=d(2, 1)),
                  f8_prod(Nqkv, D, K, 10 * l + 3, desc=d(3, 4), rseg=kvhd)]
    c = Call(tuple(prods))
    try:
        rc, sk, kern = c.group(launches=2)
        assert rc == 0, c.L.last_error()
        assert (sk, kern) == (3, K8GF)
        c.check_exact(2, "fp8 group")
    finally:
        c.close()


def test_f8_group_of_128_products(monkeypatch):
    """128 small fp8 products with distinct data and descales in one plan, two splits of one K tile each: the product field of
    gemm8p_group_f8_kernel's work word up to 127, several products per XCD list."""
    _set_arm(monkeypatch, ARMS[0], 2)
    prods = tuple(f8_prod(8 + 8 * (i % 9), 8 + 8 * (i % 5), 256, 500 + i, desc=(2.0 ** (i % 5 - 2),)) for i in range(128))
    c = Call(prods)
    try:
        rc, sk, kern = c.group()
        assert rc == 0, c.L.last_error()
        assert (sk, kern) == (2, K8GF)
        c.check_exact(1, "fp8 group of 128")
    finally:
        c.close()


# ---------------------------------------------------------------- argument errors
def _refused(c, **kw):
    rc, _, _ = c.group(**kw)
    msg = c.L.last_error()
    assert rc == ERR_ARG, (rc, msg)
    assert "grouped GEMM" in msg, msg
    np.testing.assert_array_equal(c.read(), c.C0, err_msg="a refused plan ran something")


def test_group_argument_errors(monkeypatch):
    """what gemm8p_group_plan_create refuses comes back as RSYS_ERR_ARG with a message that names the grouped GEMM, and no kernel runs"""
    _set_arm(monkeypatch, ARMS[0], None)
    lib, L = _lib()
    sk, kern = C.c_int32(-1), C.c_int32(-1)
    assert lib.rsys_op_gemm_group(0, *[None] * 13, 0, 1, C.byref(sk), C.byref(kern)) == ERR_ARG          # no product
    assert "grouped GEMM" in L.last_error(), L.last_error()
    c = Call(small_prods(3))
    try:
        _refused(c, n=129)                                           # one more than a work word's plan takes
        _refused(c, ordered=True, n=129)
    finally:
        c.close()
    bf, f8 = small_prods(1)[0], f8_prod(72, 64, 256, 0)
    c = Call((bf, f8))                                               # one form per plan
    try:
        _refused(c)
    finally:
        c.close()
    c = Call((f8, bf))
    try:
        _refused(c)
    finally:
        c.close()
    rng = np.random.default_rng(5)
    odd = Prod(_ints(rng, (64, 16)), _ints(rng, (64, 16)))           # N = 12 of a 16-wide operand
    odd.N = 12; odd.ref = odd.ref[:, :12]
    c = Call((small_prods(1)[0], odd))
    try:
        _refused(c)
    finally:
        c.close()
    c = Call((f8,))                                                  # the ordered form exists for bf16 only
    try:
        _refused(c, ordered=True)
    finally:
        c.close()
    c = Call(small_prods(2), ldc_of=lambda i, p: p.N + (2 if i == 1 else 0))   # ordered: float4 rows
    try:
        _refused(c, ordered=True)
        rc, _, kern = c.group()                                      # (the atomic arms take that stride)
        assert rc == 0 and kern == K4KG, L.last_error()
        c.check_exact(1, "ldc % 4 == 2")
    finally:
        c.close()
