"""CPU tests of the cross-rank exact sums (isfusion_amd.collectives): the big-integer model of tests/collectives_common.py
-- invariant under every permutation of the ranks, no overflow at the bound, inside a derived bound of the exact rational
mean -- the C symbols, the --data-order parser of tools/train_step.py and the mode-off path of all_reduce_sum_."""
import os
import re

import numpy as np
import pytest
import torch

import collectives_common as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("isf_fixed_absmax_tensors", "isf_fixed_pack_tensors", "isf_fixed_finish_tensors", "isf_fixed_sum_rows")


# ------------------------------------------------------------------------------------------------ the model
def test_model_is_invariant_under_every_permutation_of_the_ranks():
    rows = CM.rank_recipe(4, 1024)
    first = CM.reduce_tensor(list(rows), 4)
    cols = CM.sum_rows(rows, 4)
    for order in CM.orders(4):
        got = CM.reduce_tensor([rows[r] for r in order], 4)
        assert got[:3] == first[:3] and CM.same_bits(got[3], first[3]), order
    assert CM.same_bits(CM.sum_rows(rows[[2, 0, 3, 1]], 4), cols)
    # ... which the float sum the collectives form today is not: one rounding per add, so the order shows
    seq = [CM.sequential_sum(rows, order) for order in ((0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2))]
    assert not CM.same_bits(seq[0], seq[1]) and not CM.same_bits(seq[0], seq[2])


@pytest.mark.parametrize("world", [1, 2, 3, 4, 5, 8, 64, 100, 1000, 1024])
def test_sum_stays_below_2_62_at_the_bound(world):
    """every rank contributes +A (or every rank -A) in every element: the largest sum the bound allows"""
    top = np.array([0x7f7fffff], np.uint32).view(np.float32)[0]                      # the largest finite float32
    for a in (1.0, 0.75, 1e-9, 3.0e38, float(top), float(np.nextafter(np.float32(2.0), np.float32(0.0))), 2.0 ** -126):
        for sign in (1.0, -1.0):
            x = np.full(3, sign * a, np.float32)
            bits, e, sums, out = CM.reduce_tensor([x] * world, world)
            assert e is not None and all(abs(s) < 2 ** 62 for s in sums), (a, world, sums[0])
            assert abs(CM.pack(x, e)[0]) <= 2 ** (62 - CM.ceil_log2(world))
            assert CM.same_bits(out, x)                                                 # the mean of W equal values


@pytest.mark.parametrize("recipe", ["ranks", "ranks3", "cancelling"])
def test_model_against_the_exact_rational_mean(recipe):
    """|model - exact| <= ulp32(exact) + W * 2^-(e + 1): the roundings of the finish (a double division and one rounding
    to float32, together inside one float32 spacing) plus half a unit of 2^-e per packed contribution.  Derived, not fitted."""
    rows = {"ranks": lambda: CM.rank_recipe(4, 4096), "ranks3": lambda: CM.rank_recipe(3, 1024, seed=8),
            "cancelling": CM.cancelling_recipe}[recipe]()
    w = rows.shape[0]
    bits, e, sums, out = CM.reduce_tensor(list(rows), w)
    exact = CM.exact_mean(list(rows), w)
    for got, want in zip(out, exact):
        assert abs(float(got) - float(want)) <= CM.ulp32(want) + w * 2.0 ** -(e + 1)
    if recipe == "cancelling":                    # x - x + tiny: the float sum keeps the tiny row in one order only
        assert not CM.same_bits(CM.sequential_sum(rows, (0, 2, 1)), CM.sequential_sum(rows, (0, 1, 2)))
    if recipe == "ranks":                         # the order shows in the float sums of the issue's recipe
        assert not CM.same_bits(CM.sequential_sum(rows, (0, 1, 2, 3)), CM.sequential_sum(rows, (3, 2, 1, 0)))


def test_model_poisons_a_tensor_with_a_non_finite_contribution_and_keeps_zeros():
    rs = np.random.RandomState(3)
    good = [CM.tensor_of("unit", 7, rs) for _ in range(3)]
    for kind in ("nan", "inf"):
        bad = [good[0], CM.tensor_of(kind, 7, rs), good[2]]
        bits, e, sums, out = CM.reduce_tensor(bad, 3)
        assert bits >= CM.INF_BITS and e is None and np.isnan(out).all() and all(s == 0 for s in sums)
    zeros = CM.reduce_tensor([np.zeros(5, np.float32)] * 3, 3)
    assert zeros[0] == 0 and CM.same_bits(zeros[3], np.zeros(5, np.float32))
    rows = np.stack(good)
    rows[1, 2] = np.nan
    cols = CM.sum_rows(rows)
    assert np.isnan(cols[2]) and np.isfinite(np.delete(cols, 2)).all()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_fixed_reduce_symbols_are_declared_mirrored_and_exported():
    from isfusion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "isf_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "#define ISF_FIXED_MAX_ROWS 64" in hdr and _lib.FIXED_MAX_ROWS == 64
    nargs = {n: len(_lib.SIGNATURES[n][1]) for n in ENTRIES}
    assert nargs == {"isf_fixed_absmax_tensors": 6, "isf_fixed_pack_tensors": 7, "isf_fixed_finish_tensors": 8,
                     "isf_fixed_sum_rows": 6}
    # argument checks that need no device
    assert lib.isf_fixed_sum_rows(None, 65, 4, 1.0, None, None) != 0 and b"rows" in lib.isf_last_error()
    assert lib.isf_fixed_sum_rows(None, 3, 0, 1.0, None, None) == 0
    assert lib.isf_fixed_pack_tensors(None, None, 0, None, 11, None, None) != 0
    assert lib.isf_fixed_finish_tensors(None, None, 0, None, 3, None, 0.0, None) != 0
    assert lib.isf_fixed_pack_tensors(None, None, 0, None, 3, None, None) == 0


# ------------------------------------------------------------------------------------------------ host paths
def test_data_order_parsing():
    assert CM.parse_data_order("", 3) == [0, 1, 2]
    assert CM.parse_data_order("2,0,1", 3) == [2, 0, 1]
    assert CM.parse_data_order("0", 1) == [0]
    for bad in ("0,1", "0,1,1", "0,1,3", "a,b,c", "0,1,2,3", "-1,0,1"):
        with pytest.raises(ValueError):
            CM.parse_data_order(bad, 3)


def test_collectives_refuse_what_the_kernels_do_not_take():
    from isfusion_amd import collectives
    from isfusion_amd._lib import IsfError
    assert [collectives.ceil_log2(n) for n in (1, 2, 3, 4, 5, 8, 9, 1024)] == [0, 1, 2, 2, 3, 3, 4, 10]
    with pytest.raises(IsfError):
        collectives.sum_rows(torch.zeros(3, 4))                                          # a CPU tensor: no fallback
    with pytest.raises(IsfError):
        collectives.TensorTable([torch.zeros(4)])


def test_all_reduce_sum_with_the_mode_off_is_the_plain_all_reduce(tmp_path):
    """one gloo rank, mode off: dist.all_reduce on the tensor itself -- the input's bits come back, on a CPU tensor too;
    with `exact` a single rank takes the same call"""
    import torch.distributed as dist
    from isfusion_amd import collectives, norm
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/rendezvous", rank=0, world_size=1)
    try:
        x = torch.from_numpy(CM.rank_recipe(1, 257)[0])
        for exact in (False, True):
            t = x.clone()
            assert collectives.all_reduce_sum_(t, exact) is t and CM.same_bits(t.numpy(), x.numpy())
        y = norm._AllReduceSum.apply(x.clone().requires_grad_())
        y.backward(torch.ones_like(y))
        assert CM.same_bits(y.detach().numpy(), x.numpy())
    finally:
        dist.destroy_process_group()
