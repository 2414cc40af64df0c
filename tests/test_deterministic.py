"""CPU tests of the deterministic mode: the fixed-point accumulation rule of the isf_*_det entries restated in numpy
(tests/det_common.py) and the three API calls.  That the four new entries are declared in include/isf_hip.h, listed in
_lib.SIGNATURES and exported by the built library is already checked by tests/test_host.py (declared == SIGNATURES, every
signature resolves): nothing is added for it here."""
import importlib.util
import math
import os

import numpy as np
import pytest

import det_common as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- 1. the fixed-point sum
def test_exponent_rule():
    """e = 62 - ceil(log2 N) - ex, A < 2^ex: a power of two takes the next exponent, zero takes 0"""
    assert DC.fixed_exponent(np.float32(1.0), 1) == 62 - 0 - 1
    assert DC.fixed_exponent(np.float32(0.75), 4096) == 62 - 12 - 0
    assert DC.fixed_exponent(np.float32(4096.0), 4099) == 62 - 13 - 13
    assert DC.fixed_exponent(np.float32(0.0), 8) == 62 - 3
    assert DC.fixed_exponent(np.float32(2.0 ** -140), 2) == 62 - 1 + 139          # subnormal bounds too
    assert [DC.ceil_log2(n) for n in (1, 2, 3, 4, 5, 4096, 4097)] == [0, 1, 2, 2, 3, 12, 13]


def test_three_values_whose_float_sum_depends_on_the_order():
    v = np.array([1.0, 2.0 ** -30, -1.0], np.float32)
    float_sums = set()
    for order in ([0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]):
        s = np.float32(0)
        for i in order:
            s = np.float32(s + v[i])
        float_sums.add(float(s))
        assert DC.fixed_sum(v[order]) == np.float32(2.0 ** -30)
    assert float_sums == {0.0, 2.0 ** -30}


def test_sum_is_unchanged_by_permutations_and_is_the_exact_sum():
    rng = np.random.default_rng(7)
    v = DC.pow2_values(rng, 4096)
    want = DC.fixed_sum(v)
    # resolution 2^-(62 - 12 - 13) = 2^-37 is below the last bit of the smallest value (2^-12 * 2^-23): every q is exact
    assert want == np.float32(math.fsum(float(x) for x in v))
    for _ in range(20):
        assert DC.fixed_sum(v[rng.permutation(v.size)]).tobytes() == want.tobytes()
    # several accumulators at once (axis 0), as the kernels use it
    m = DC.pow2_values(rng, (300, 5))
    assert DC.fixed_sum(m[rng.permutation(300)]).tobytes() == DC.fixed_sum(m).tobytes()


def test_zero_bound_gives_zeros():
    out = DC.fixed_sum(np.zeros((17, 3), np.float32))
    assert out.shape == (3,) and not out.any() and not np.signbit(out).any()


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_non_finite_bound_makes_every_output_nan(bad):
    v = np.ones((9, 4), np.float32)
    v[3, 1] = bad
    assert not np.isfinite(DC.absmax_f32(v))
    assert np.isnan(DC.fixed_sum(v)).all()
    cmap = np.array([0, 0, 1, 1, -1, 2, 2, 2, 0])
    assert np.isnan(DC.scatter_sum(v, cmap, 3)).all()


@pytest.mark.parametrize("N", [1, 2, 4099, 257 * 12, 70 * 16, 1 << 21])
@pytest.mark.parametrize("A", [1.0, 0.75, 2.0 ** 12, float(np.nextafter(np.float32(2.0 ** 12), np.float32(0))), 3e38, 1e-40])
def test_no_overflow_at_the_documented_n(N, A):
    """N contributions all equal to the bound A stay inside int64, and come back as N * A"""
    A = np.float32(A)
    e = DC.fixed_exponent(A, N)
    q = int(DC.quantize(A, e))
    assert abs(q) <= 1 << (62 - DC.ceil_log2(N))
    total = q * N                                             # Python int: no wrap
    assert abs(total) <= 1 << 62 < (1 << 63) - 1
    assert np.int64(total) == total
    if N <= 4099:
        s = DC.fixed_sum(np.full(N, A, np.float32), N=N)
        if np.isfinite(np.float64(A) * N) and np.float64(A) * N < 3.4e38:
            assert s == np.float32(np.float64(A) * N)


def test_scatter_restatement_groups_rows():
    feats, coors = DC.scatter_case(3)
    assert ((coors < 0).any(1)).sum() == 40
    valid = coors[(coors >= 0).all(1)]
    uniq, counts = np.unique(valid, axis=0, return_counts=True)
    assert len(uniq) == 20 and sorted(counts)[-3:] == [1347, 1347, 1348] and sorted(counts)[:17] == [1] * 17


# ------------------------------------------------------------------------------------------- 2. the API
def test_api_default_nesting_and_restore():
    import isfusion_amd as m
    assert m.is_deterministic() is False
    with m.deterministic():
        assert m.is_deterministic()
        with m.deterministic(False):
            assert not m.is_deterministic()
            with m.deterministic(True):
                assert m.is_deterministic()
            assert not m.is_deterministic()
        assert m.is_deterministic()
    assert not m.is_deterministic()
    with pytest.raises(ValueError):
        with m.deterministic():
            raise ValueError("inside")
    assert not m.is_deterministic()
    m.set_deterministic(True)
    try:
        assert m.is_deterministic()
        with m.deterministic(False):
            assert not m.is_deterministic()
        assert m.is_deterministic()                           # back to what set_deterministic left
    finally:
        m.set_deterministic(False)
    assert not m.is_deterministic()


def test_api_needs_neither_gpu_nor_library():
    """the module that holds the flag imports nothing: loaded on its own from its file, with no package around it"""
    path = os.path.join(ROOT, "is-fusion_amd", "determinism.py")
    spec = importlib.util.spec_from_file_location("determinism_alone", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert not mod.is_deterministic()
    assert mod.entry("isf_p2g_backward") == "isf_p2g_backward"
    with mod.deterministic():
        assert mod.is_deterministic() and mod.entry("isf_p2g_backward") == "isf_p2g_backward_det"
    assert not mod.is_deterministic()
    src = open(path).read()
    assert "import torch" not in src and "_lib" not in src


def test_mode_asks_the_stock_convolutions_for_deterministic_algorithms_and_restores():
    import torch
    import isfusion_amd as m
    for before in (False, True):
        torch.backends.cudnn.deterministic = before
        try:
            with m.deterministic():
                assert torch.backends.cudnn.deterministic is True
                with m.deterministic(False):
                    assert torch.backends.cudnn.deterministic is before
                assert torch.backends.cudnn.deterministic is True
            assert torch.backends.cudnn.deterministic is before
        finally:
            torch.backends.cudnn.deterministic = False


def test_entries_follow_the_flag():
    from isfusion_amd import _lib, determinism
    for name in ("isf_dynamic_point_to_voxel_forward", "isf_p2g_backward", "isf_msda_backward",
                 "isf_ms_deform_attn_backward"):
        assert determinism.entry(name) == name
        with determinism.deterministic():
            assert determinism.entry(name) == name + "_det"
            assert _lib.SIGNATURES[name + "_det"] == _lib.SIGNATURES[name]      # the sibling's argument list
