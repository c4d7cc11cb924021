"""GPU: the scoring of a request's text queries alone (rsys_op_text_rows: text_scores_kernel and the log-sum-exp launches of rsys_op_lse
behind the upload and projection of rsys_search_topk; csrc/search.hip) against tests/_search_np.logp plus its logsumexp.
Operand scales (_A), the comparison (_relerr) and the bounds (TOL, relative) are those of tests/test_gpu_search_ragged.py.

Shapes: item counts of 1, around one wave step of 4 x 4 rows and one workgroup of 64 rows (63, 64, 65), around the 256-row padding of the
table (255, 257), 1025 and 3001 (many item blocks, the last one ragged); D = 64 (8 lanes of a wave hold a bf16 row), 192 (no power of
two), 2048 (the 64 KiB LDS tile of 8 texts) and 4096 (the tile halves to 4 texts); n = 1, 7, 8, 9, 17 texts (the 1-text tile, a ragged
tile, a full tile, two tiles, three tiles -- five at D = 4096); logit_scale 1 and 5; both dtypes.  D = 3072 and 4608 are widths at
which 64 KiB hold a number of fp32 rows that is no power of two (5 and 3): the tile must round down to 4 and 2 texts, at n = 5, 9, 17
(n above the rows that fit: two, three and five tiles at 3072; three, five and nine at 4608)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _search_np as sn  # noqa: E402
from test_gpu_search import _A, _relerr  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-4, "bf16": 1e-3}
NS = (1, 7, 8, 9, 17)


def _model(dtype, v, d, q, s=1.0, seed=0):
    """test_gpu_search._model with max_batch = 64"""
    from recommendersystem_amd import search
    rng = np.random.default_rng(seed)
    feat = (rng.standard_normal((v, d)) / np.sqrt(d)).astype(np.float32)
    m = search.SearchModel(search.training_config({0: v}, batch_size=64, embed_dim=d, query_dim=q), 0, feat, dtype=dtype, max_batch=64)
    W = (rng.standard_normal((q, d)) * _A[dtype][s] / np.sqrt(q)).astype(np.float32)
    m.param_set("encoder.weight", W)
    m.param_set("logit_scale", s)
    return m, feat, W


def _check(m, feat, W, s, dtype, v, q, seed, NS=NS):
    x_all = np.random.default_rng(seed).standard_normal((max(NS), q)).astype(np.float32)
    for n in NS:
        x = x_all[:n]
        z, lse = m.text_rows(x)
        assert z.shape == (n, v) and np.isfinite(z).all() and np.isfinite(lse).all()
        z2, lse2 = m.text_rows(x)
        assert z.tobytes() == z2.tobytes() and lse.tobytes() == lse2.tobytes()                    # two calls, equal bits
        Em, Wq, xq = (sn.bf16(feat), sn.bf16(W), sn.bf16(x)) if dtype == "bf16" else (feat.astype(np.float64), W.astype(np.float64), x)
        P = xq.astype(np.float64) @ Wq
        zr = (sn.bf16(P) if dtype == "bf16" else P) @ Em.T * np.exp(s)
        ref_lse = sn.logsumexp(zr)
        ref_lp = sn.logp(feat, W, s, x, bf16_mode=dtype == "bf16")
        lp = z - lse[:, None]
        errs = {"z": max(_relerr(z[t], zr[t]) for t in range(n)), "lse": _relerr(lse, ref_lse),
                "logp": 0.0 if v == 1 else max(_relerr(lp[t], ref_lp[t]) for t in range(n))}
        print(f"{dtype} V={v} D={m.D} Q={q} s={s} n={n}", {k: f"{e:.2e}" for k, e in errs.items()})
        for k, e in errs.items():
            assert e < TOL[dtype], (k, e, n)
        if v == 1:
            assert not lp.any()                                                                   # one item holds all the mass: exactly 0
        # every tile size gives the bits of the one-text tile
        if n == max(NS):
            z1, lse1 = m.text_rows(x[4:5])
            assert z1.tobytes() == z[4:5].tobytes() and lse1.tobytes() == lse[4:5].tobytes()
        # per id against the handle's own top-k (the 256-row GEMM path), within the same bound
        if n in (1, 9):
            ids, tlp = m.topk(x, v)
            for t in range(n):
                assert sorted(ids[t]) == list(range(v))
                got = np.empty(v, np.float64)
                got[ids[t]] = tlp[t]
                assert v == 1 and not got.any() or _relerr(lp[t], got) < TOL[dtype], (t, _relerr(lp[t], got))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("v", [1, 63, 64, 65, 255, 257, 1025, 3001])
def test_item_counts(v, dtype):
    m, feat, W = _model(dtype, v, 64, 64, seed=v)
    _check(m, feat, W, 1.0, dtype, v, 64, seed=100 + v)
    m.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("d,q", [(192, 192), (2048, 64), (4096, 64)])
@pytest.mark.parametrize("v", [257, 3001])
def test_widths(v, d, q, dtype):
    m, feat, W = _model(dtype, v, d, q, seed=d + v)
    _check(m, feat, W, 1.0, dtype, v, q, seed=200 + d + v)
    m.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("d,q", [(64, 64), (192, 192)])
def test_logit_scale_5(d, q, dtype):
    m, feat, W = _model(dtype, 1025, d, q, s=5.0, seed=5 + d)
    _check(m, feat, W, 5.0, dtype, 1025, q, seed=300 + d)
    m.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("d", [3072, 4608])
def test_widths_whose_lds_rows_are_no_power_of_two(d, dtype):
    m, feat, W = _model(dtype, 257, d, 64, seed=d)
    _check(m, feat, W, 1.0, dtype, 257, 64, seed=400 + d, NS=(5, 9, 17))
    m.close()


def test_argument_rules():
    from recommendersystem_amd import search
    from recommendersystem_amd._lib import lib
    L = lib()
    m, feat, W = _model("fp32", 65, 64, 64)
    x = np.zeros((65, 64), np.float32)
    z = np.full((65, 65), -7, np.float32); lse = np.full(65, -7, np.float32)
    for n in (0, -1, 65):
        assert L.rsys_op_text_rows(m.h, x.ctypes.data, n, z.ctypes.data, lse.ctypes.data) == -1
    x[3, 5] = np.nan
    assert L.rsys_op_text_rows(m.h, x.ctypes.data, 4, z.ctypes.data, lse.ctypes.data) == -1
    assert L.rsys_op_text_rows(m.h, None, 4, z.ctypes.data, lse.ctypes.data) == -1
    assert (z == -7).all() and (lse == -7).all()
    m.close()
    small = search.SearchModel(search.training_config({0: 65}, batch_size=4, embed_dim=64, query_dim=64), 0, feat, dtype="fp32", max_batch=4)
    small.init_weights()
    assert L.rsys_op_text_rows(small.h, x.ctypes.data, 5, z.ctypes.data, lse.ctypes.data) == -1     # more texts than the handle's max_batch
    small.close()
