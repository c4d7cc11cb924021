"""CPU: which GEMM kernel launch_gemm runs, and with how many K splits, for concrete problems (rsys_debug_gemm_route: the host-side
routing of csrc/gemm.hip, no launch).  The table pins the routing rules of gemm.hip, gemm8p.hip, gemm8c.hip, gemm4p.hip and
gemm4k.hip as measured and tuned; a change to any of them shows up here as a changed row."""
import ctypes as C
import os

import pytest

EPI_STORE, EPI_ACCUM, EPI_ATOMIC, EPI_BIAS, EPI_QKV_ROPE = 0, 1, 2, 3, 5
M_DEV, K_DEV, SLAB, ROPE_CS, ROPE_POS, C2 = 1, 2, 4, 8, 16, 32
BF16, FP32 = 1, 0
GEMM_SWITCHES = ("RSYS_GEMM_KERNEL", "RSYS_GEMM_KERNEL_TN", "RSYS_GEMM_KERNEL_NT_SPLITK", "RSYS_GEMM_KERNEL_MIX", "RSYS_GEMM4P",
                 "RSYS_GEMM4K", "RSYS_GEMM8C", "RSYS_DEBUG_8P", "RSYS_DEBUG_8T_SPLITK")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    from recommendersystem_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


@pytest.fixture(autouse=True)
def default_switches(L, monkeypatch):
    """Every case starts from the default switches; the environment and the parsed switches are restored afterwards."""
    for name in GEMM_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    L.rsys_switches_reload()
    yield
    monkeypatch.undo()
    L.rsys_switches_reload()


def route(L, M, N, K, *, dtype=BF16, a_km=0, b_km=0, a_f32=0, c_f32=0, epi=EPI_STORE, splitk=1, flags=0, alpha=1.0, accum=0,
          ptrs=0, m_expect=0, cus=256):
    lda = M if a_km else K
    ldb = N if b_km else K
    lda, ldb = (lda + 7) // 8 * 8, (ldb + 7) // 8 * 8
    tag = C.create_string_buffer(16)
    splits = C.c_int32(0)
    rc = L.rsys_debug_gemm_route(dtype, M, N, K, lda, ldb, N, a_km, b_km, a_f32, c_f32, epi, splitk, flags, alpha, accum, ptrs,
                                 m_expect, cus, tag, len(tag), C.byref(splits))
    assert rc == 0
    return tag.value.decode(), splits.value


ATOMIC_KM = dict(a_km=1, b_km=1, c_f32=1, epi=EPI_ATOMIC, splitk=4)   # a weight gradient dW = dY^T X (K = tokens)
STORE_KM = dict(a_km=1, b_km=1, c_f32=1, epi=EPI_STORE)              # the tied head's table gradient form
ATOMIC_NT = dict(c_f32=1, epi=EPI_ATOMIC, splitk=3)                 # row-major operands, split-K atomics
MIX = dict(b_km=1, c_f32=1, epi=EPI_ATOMIC, splitk=8, ptrs=M_DEV)    # the tied head's dEw = dlogits . F over device-side live rows

# (id, (M, N, K), options, expected (tag, K splits))
CASES = [
    # pick_rowmajor_kernel: 256x256 family from 128 tiles of 256 x 256 on; gemm8c takes the plain store
    ("rowmajor_t256_128_8c", (4096, 2048, 1024), {}, ("8c", 1)),
    ("rowmajor_t256_120_nt", (3840, 2048, 1024), {}, ("nt", 1)),
    # gemm8c's epilogue classes: bias stays on gemm8p; RoPE needs the interleaved table on the 256x256 family and no explicit positions for gemm8c
    ("rowmajor_bias_8p", (4096, 2048, 1024), dict(epi=EPI_BIAS, c_f32=1), ("8p", 1)),
    ("rowmajor_rope_no_cs_nt", (4096, 2048, 1024), dict(epi=EPI_QKV_ROPE), ("nt", 1)),
    ("rowmajor_rope_cs_8c", (4096, 2048, 1024), dict(epi=EPI_QKV_ROPE, ptrs=ROPE_CS), ("8c", 1)),
    ("rowmajor_rope_pos_8p", (4096, 2048, 1024), dict(epi=EPI_QKV_ROPE, ptrs=ROPE_CS | ROPE_POS), ("8p", 1)),
    # gemm8p_eligible: no accumulate-into-T, no device-side K limit
    ("rowmajor_accum_nt", (4096, 2048, 1024), dict(accum=1), ("nt", 1)),
    ("rowmajor_k_dev_nt", (4096, 2048, 1024), dict(ptrs=K_DEV), ("nt", 1)),
    # m_expect: the device-side row limit's host estimate sets the tile count (3000 rows: 96 tiles)
    ("m_expect_below_128_nt", (4096, 2048, 1024), dict(ptrs=M_DEV, m_expect=3000), ("nt", 1)),
    ("m_dev_no_expect_8c", (4096, 2048, 1024), dict(ptrs=M_DEV), ("8c", 1)),
    # use_4p: K >= 8192, N >= 1024 and >= 256 whole tiles, and just below each bound
    ("4p_at_bounds", (8192, 2048, 8192), {}, ("4p", 1)),
    ("4p_k_below", (8192, 2048, 8064), {}, ("8c", 1)),
    ("4p_n_below", (22016, 768, 8192), {}, ("8c", 1)),
    ("4p_tiles_below", (7936, 2048, 8192), {}, ("8c", 1)),
    ("4p_not_with_m_dev", (8192, 2048, 8192), dict(ptrs=M_DEV), ("8c", 1)),
    # use_8p_tn: K-major atomic from 16 tiles on, on gemm4k; a slab (deterministic mode) keeps gemm8p's kernel; K splits from gemm8p_splits
    ("km_atomic_t256_16_4k", (1024, 1024, 16384), ATOMIC_KM, ("4k", 16)),
    ("km_atomic_slab_8t", (1024, 1024, 16384), dict(ATOMIC_KM, ptrs=SLAB), ("8t", 16)),
    ("km_atomic_t256_12_tn", (1024, 768, 16384), ATOMIC_KM, ("tn", 8)),
    # use_8p_tn_store: K-major fp32 store from 128 tiles on
    ("km_store_t256_128_8ts", (4096, 2048, 1024), STORE_KM, ("8ts", 1)),
    ("km_store_t256_120_tn", (3840, 2048, 1024), STORE_KM, ("tn", 1)),
    # use_8p_nt_splitk: row-major atomic from 32 tiles on, or from 8 with K * tiles >= 32 * 16384; flags bit 7 forces it
    ("nt_splitk_32_tiles_8s", (1024, 2048, 2048), ATOMIC_NT, ("8s", 8)),
    ("nt_splitk_28_tiles_nt", (1024, 1792, 2048), ATOMIC_NT, ("nt", 8)),
    ("nt_splitk_8_tiles_long_k_8s", (512, 1024, 65536), ATOMIC_NT, ("8s", 32)),
    ("nt_splitk_6_tiles_long_k_nt", (512, 768, 65536), ATOMIC_NT, ("nt", 8)),
    ("nt_splitk_flag_bit7_8s", (256, 256, 2048), dict(ATOMIC_NT, flags=128), ("8s", 24)),
    ("nt_atomic_short_k_nt", (4096, 2048, 512), ATOMIC_NT, ("nt", 8)),
    # use_8p_mix: K >= 8192 and N >= 512 (K rounded down to 64 for the kernel, the tail on the 128x128 one); N = 256 stays on nn
    ("mix_8m", (512, 512, 100000), MIX, ("8m", 8)),
    ("mix_n256_nn", (512, 256, 100000), MIX, ("nn", 8)),
    ("mix_k_below_nn", (512, 512, 8000), MIX, ("nn", 8)),
    ("mix_slab_nn", (512, 512, 100000), dict(MIX, ptrs=M_DEV | SLAB), ("nn", 8)),
    # operands stored as fp32 and the fp32 compute type stay on the 128x128 kernel
    ("a_f32_nt", (4096, 2048, 1024), dict(a_f32=1), ("nt", 1)),
    ("fp32_nt", (4096, 2048, 1024), dict(dtype=FP32, c_f32=1), ("nt", 1)),
    ("fp32_km_atomic_tn", (1024, 1024, 16384), dict(ATOMIC_KM, dtype=FP32), ("tn", 8)),
    ("fp32_mix_nn", (512, 512, 100000), dict(MIX, dtype=FP32), ("nn", 8)),
]


@pytest.mark.parametrize("shape,opts,want", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_route_table(L, shape, opts, want):
    assert route(L, *shape, **opts) == want


# the forcing arm of every GEMM switch: (id, {switch: value}, (M, N, K), options, expected)
SWITCH_CASES = [
    # RSYS_GEMM_KERNEL=1: the 128x128 kernel everywhere (also for the mixed layout); 2: the 256x256 family wherever eligible
    ("gemm_kernel_1_nt", {"RSYS_GEMM_KERNEL": "1"}, (4096, 2048, 1024), {}, ("nt", 1)),
    ("gemm_kernel_1_mix_nn", {"RSYS_GEMM_KERNEL": "1"}, (512, 512, 100000), MIX, ("nn", 8)),
    ("gemm_kernel_2_8c", {"RSYS_GEMM_KERNEL": "2"}, (256, 256, 1024), {}, ("8c", 1)),
    # RSYS_GEMM_KERNEL_TN=1: never the K-major LDS-DMA kernels; 2: both their forms wherever eligible
    ("tn_1_atomic_tn", {"RSYS_GEMM_KERNEL_TN": "1"}, (1024, 1024, 16384), ATOMIC_KM, ("tn", 8)),
    ("tn_1_store_tn", {"RSYS_GEMM_KERNEL_TN": "1"}, (4096, 2048, 1024), STORE_KM, ("tn", 1)),
    ("tn_2_atomic_4k", {"RSYS_GEMM_KERNEL_TN": "2"}, (512, 512, 16384), ATOMIC_KM, ("4k", 56)),
    ("tn_2_store_8ts", {"RSYS_GEMM_KERNEL_TN": "2"}, (256, 256, 1024), STORE_KM, ("8ts", 1)),
    # RSYS_GEMM_KERNEL_NT_SPLITK=2: the row-major split-K form whatever the tile count
    ("nt_splitk_2_8s", {"RSYS_GEMM_KERNEL_NT_SPLITK": "2"}, (256, 256, 2048), ATOMIC_NT, ("8s", 24)),
    # RSYS_GEMM_KERNEL_MIX=0: never; 2: wherever eligible
    ("mix_0_nn", {"RSYS_GEMM_KERNEL_MIX": "0"}, (512, 512, 100000), MIX, ("nn", 8)),
    ("mix_2_8m", {"RSYS_GEMM_KERNEL_MIX": "2"}, (512, 256, 8000), MIX, ("8m", 8)),
    # RSYS_GEMM4P=0: never; 2: wherever eligible
    ("gemm4p_0_8c", {"RSYS_GEMM4P": "0"}, (8192, 2048, 8192), {}, ("8c", 1)),
    ("gemm4p_2_4p", {"RSYS_GEMM4P": "2"}, (4096, 2048, 1024), {}, ("4p", 1)),
    # RSYS_GEMM4K=0: K-major split-K products on gemm8p's kernel
    ("gemm4k_0_8t", {"RSYS_GEMM4K": "0"}, (1024, 1024, 16384), ATOMIC_KM, ("8t", 16)),
    # RSYS_GEMM8C=0: the row-major 256x256 products on gemm8p (gemm4p is reached through gemm8c only)
    ("gemm8c_0_8p", {"RSYS_GEMM8C": "0"}, (4096, 2048, 1024), {}, ("8p", 1)),
    ("gemm8c_0_long_k_8p", {"RSYS_GEMM8C": "0"}, (8192, 2048, 8192), {}, ("8p", 1)),
    # RSYS_DEBUG_8P (timing flags) keeps gemm8p's own kernel
    ("debug_8p_8p", {"RSYS_DEBUG_8P": "1"}, (4096, 2048, 1024), {}, ("8p", 1)),
    # RSYS_DEBUG_8T_SPLITK: the K-major split count, rounded up to a multiple of 8; the row-major split-K form ignores it
    ("debug_8t_splitk_4k", {"RSYS_DEBUG_8T_SPLITK": "20"}, (1024, 1024, 16384), ATOMIC_KM, ("4k", 24)),
    ("debug_8t_splitk_8s", {"RSYS_DEBUG_8T_SPLITK": "20"}, (1024, 2048, 2048), ATOMIC_NT, ("8s", 8)),
]


@pytest.mark.parametrize("env,shape,opts,want", [c[1:] for c in SWITCH_CASES], ids=[c[0] for c in SWITCH_CASES])
def test_route_switches(L, monkeypatch, env, shape, opts, want):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L.rsys_switches_reload()
    assert route(L, *shape, **opts) == want


def test_cus_does_not_move_the_route(L):
    # the tile-count rules are written for the MI355X's 256 CUs as measured; the CU count the route is given does not change them
    for cus in (80, 256, 304):
        assert route(L, 4096, 2048, 1024, cus=cus) == ("8c", 1)
        assert route(L, 1024, 1024, 16384, cus=cus, **ATOMIC_KM) == ("4k", 16)
