"""GPU: the log-sum-exp kernels of the retrieval scoring alone (rsys_op_lse: lse_partial_kernel, lse_final_kernel) against the fp64
log-sum-exp of the same float32 rows.  The tolerance is four times the worst error of the float32 restatement of the kernels' fold
order over the same rows (tests/_retrieve_np.py LSE_RESTATED_ERR, measured by test_retrieve_select_host.py): the device's expf and logf
differ from numpy's by a few ulp per term.  Measured on an MI355X over the cases below, worst |error| per kind of row: random 7.0e-07,
equal 1.5e-06 (V = 119999: the device's logf(119999) is two ulp below the correctly rounded value), ascending 7.2e-07, descending
7.4e-07, spike 0, near_88 4.2e-06, near_m100 4.3e-06, inf_stripe 7.0e-07; the restatement's: 4.1e-06 (near_88)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _retrieve_np as rn  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_ARG = -1                     # RSYS_ERR_ARG
LSE_TOL = 4.0 * max(rn.LSE_RESTATED_ERR.values())      # 4 x 4.1e-06 (the restatement, near_88) = 1.64e-05; the device's worst: 4.3e-06


def _op_lse(z, ldz=None):
    from recommendersystem_amd._lib import check, lib
    L = lib()
    rows, V = z.shape
    ldz = V if ldz is None else ldz
    host = np.full((rows, ldz), np.nan, np.float32)
    host[:, :V] = z
    pz, po = C.c_void_p(), C.c_void_p()
    check(L.rsys_dev_alloc(C.byref(pz), host.nbytes))
    check(L.rsys_dev_alloc(C.byref(po), rows * 4))
    try:
        check(L.rsys_dev_h2d(pz, host.ctypes.data, host.nbytes))
        out = []
        for _ in range(2):                                       # the same call twice: identical bits
            check(L.rsys_dev_memset(po, 0x5a, rows * 4))
            check(L.rsys_op_lse(pz, ldz, rows, V, po))
            got = np.empty(rows, np.float32)
            check(L.rsys_dev_d2h(got.ctypes.data, po, got.nbytes))
            out.append(got)
    finally:
        L.rsys_dev_free(pz)
        L.rsys_dev_free(po)
    assert out[0].tobytes() == out[1].tobytes()
    return out[0]


@pytest.mark.parametrize("rows", rn.LSE_ROWS)
@pytest.mark.parametrize("V", rn.LSE_VS)
def test_lse_against_fp64(V, rows):
    z, kinds = rn.lse_case(V, rows)
    ref = rn.lse_fp64(z)
    got = _op_lse(z)
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    worst = {}
    for r, k in enumerate(kinds):
        worst[k] = max(worst.get(k, 0.0), float(err[r]))
    print("lse", V, rows, {k: f"{v:.3e}" for k, v in worst.items()})
    for r, k in enumerate(kinds):
        assert err[r] <= LSE_TOL, (V, rows, r, k, float(err[r]), LSE_TOL, float(got[r]), float(ref[r]))


def test_lse_row_stride():
    z, kinds = rn.lse_case(129, 3)
    assert _op_lse(z, ldz=200).tobytes() == _op_lse(z).tobytes()      # NaN in the padding columns is never read


def test_lse_leading_inf_stripe_resets_the_running_sum():
    """3000 leading -inf: a lane's running sum is NaN (expf(-inf - -inf)) until its first finite entry resets it; whole slices of -inf
    fold to nothing.  The result is the log-sum-exp of the finite tail alone."""
    rng = np.random.default_rng(8)
    for V in (3001, 3064, 16385, 119999):
        tail = rn.lse_rows("random", 2, V - 3000, rng)
        z = np.concatenate([np.full((2, 3000), -np.inf, np.float32), tail], axis=1)
        got = _op_lse(z)
        assert np.isfinite(got).all()
        assert (np.abs(got - rn.lse_fp64(tail)) <= LSE_TOL).all(), V


def test_lse_of_an_all_inf_row_is_minus_inf():
    """What rsys_debug.h documents: no partial has a finite max, lse_final_kernel's (m, s) stay (-inf, 0) and -inf + logf(0) = -inf."""
    for V in (1, 37, 64, 3000, 16385):
        z = np.full((3, V), -np.inf, np.float32)
        z[1] = rn.lse_rows("random", 1, V, np.random.default_rng(V))[0]
        got = _op_lse(z)
        assert np.isneginf(got[0]) and np.isneginf(got[2]) and np.isfinite(got[1]), (V, got)


def test_lse_argument_errors_leave_the_output_alone():
    from recommendersystem_amd._lib import check, lib
    L = lib()
    pz, po = C.c_void_p(), C.c_void_p()
    check(L.rsys_dev_alloc(C.byref(pz), 2 * 16 * 4))
    check(L.rsys_dev_alloc(C.byref(po), 8))
    try:
        check(L.rsys_dev_memset(pz, 0, 2 * 16 * 4))
        check(L.rsys_dev_memset(po, 0x5a, 8))
        for ldz, rows, V in ((16, 0, 16), (16, 65536, 16), (16, 2, 0), (15, 2, 16)):
            assert L.rsys_op_lse(pz, ldz, rows, V, po) == ERR_ARG
        assert L.rsys_op_lse(None, 16, 2, 16, po) == ERR_ARG
        assert L.rsys_op_lse(pz, 16, 2, 16, None) == ERR_ARG
        got = np.empty(8, np.uint8)
        check(L.rsys_dev_d2h(got.ctypes.data, po, 8))
        assert (got == 0x5a).all()
    finally:
        L.rsys_dev_free(pz)
        L.rsys_dev_free(po)
