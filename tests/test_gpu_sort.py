"""The library's stable sort on its own (csrc/isf_sort.hip through isf_debug_stable_sort) against numpy's stable argsort of
the masked keys: the order depends on the low key_bits bits and on nothing above them, equal keys keep their input order,
and a sort that continues an earlier order gives the lexicographic order of the two key columns.  Row counts: one lane, the
64-lane sub-tile edge, the 1024-row wave tile edge, the workgroup edge of four tiles, and a ragged last tile."""
import numpy as np
import pytest
import torch

from isfusion_amd import _lib

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, 5121)
KEY_BITS = (1, 5, 10, 11, 20, 21, 22, 31, 32)
ERR_ARG = -1
POISON = -7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def mask_of(key_bits):
    return np.uint32((1 << key_bits) - 1)


def sort_rc(dev, keys, key_bits, after=None, want_keys=False, num=None):
    """(return code, order, keys_sorted or None); the outputs are poisoned first"""
    n = len(keys) if num is None else num
    d_keys = torch.from_numpy(keys.view(np.int32).copy()).to(dev)
    d_after = None if after is None else torch.from_numpy(after.astype(np.int32)).to(dev)
    order = torch.full((max(len(keys), 1),), POISON, dtype=torch.int32, device=dev)
    ks = torch.full((max(len(keys), 1),), POISON, dtype=torch.int32, device=dev) if want_keys else None
    rc = _lib.load().isf_debug_stable_sort(_lib.ptr(d_keys), n, key_bits, _lib.ptr(d_after), _lib.ptr(order), _lib.ptr(ks),
                                           _lib.stream())
    torch.cuda.synchronize()
    return rc, order.cpu().numpy()[:len(keys)], None if ks is None else ks.cpu().numpy().view(np.uint32)[:len(keys)]


def sort(dev, keys, key_bits, **kw):
    rc, order, ks = sort_rc(dev, keys, key_bits, **kw)
    _lib.check(rc, "isf_debug_stable_sort")
    return order, ks


@pytest.mark.parametrize("key_bits", KEY_BITS)
@pytest.mark.parametrize("n", ROWS)
def test_order_is_the_stable_order_of_the_masked_keys(dev, n, key_bits):
    rng = np.random.default_rng(1000 * n + key_bits)
    m = mask_of(key_bits)
    # every bit random: what lies above key_bits is noise that must not decide
    noise = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    order, ks = sort(dev, noise, key_bits, want_keys=True)
    assert np.array_equal(order, np.argsort(noise & m, kind="stable"))
    assert np.array_equal(ks, noise[order])
    equal = np.full(n, 0x9E3779B9, np.uint32)
    order, _ = sort(dev, equal, key_bits)
    assert np.array_equal(order, np.arange(n))
    falling = (np.uint32(0xFFFFFFFF) - np.arange(n, dtype=np.uint32) * np.uint32(0xFFFFFFFF // n)).astype(np.uint32)
    assert np.all(falling[1:] < falling[:-1])
    order, ks = sort(dev, falling, key_bits, want_keys=True)
    assert np.array_equal(order, np.argsort(falling & m, kind="stable"))
    assert np.array_equal(ks, falling[order])


@pytest.mark.parametrize("bits1,bits2", [(32, 5), (32, 32)])
@pytest.mark.parametrize("n", (65, 4097))
def test_continuing_an_order_sorts_two_key_columns_lexicographically(dev, n, bits1, bits2):
    rng = np.random.default_rng(n + bits2)
    # the minor column repeats values, so that rows tie in both columns and the input order has to survive two sorts
    pool = rng.integers(0, 1 << 32, n // 4 + 1, dtype=np.uint64).astype(np.uint32)
    k1 = pool[rng.integers(0, len(pool), n)]
    k2 = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if bits2 == 32:
        k2 = (k2 & np.uint32(0xC0000003)).astype(np.uint32)      # few values, on both ends of the word
    first, _ = sort(dev, k1, bits1)
    order, ks = sort(dev, k2, bits2, after=first, want_keys=True)
    want = np.lexsort((k1 & mask_of(bits1), k2 & mask_of(bits2)))
    assert np.array_equal(order, want)
    assert np.array_equal(ks, k2[order])


def test_refusals_write_nothing(dev):
    keys = np.arange(100, dtype=np.uint32)
    for key_bits in (0, 33):
        rc, order, ks = sort_rc(dev, keys, key_bits, want_keys=True)
        assert rc == ERR_ARG
        assert np.all(order == POISON) and np.all(ks.view(np.int32) == POISON)
    rc, order, _ = sort_rc(dev, keys, 8, num=-1)
    assert rc == ERR_ARG and np.all(order == POISON)
    rc, order, _ = sort_rc(dev, keys, 8, num=0)
    assert rc == _lib.ISF_OK and np.all(order == POISON)
    lib = _lib.load()
    assert lib.isf_debug_stable_sort(None, 0, 8, None, None, None, _lib.stream()) == _lib.ISF_OK
    assert lib.isf_debug_stable_sort(None, 4, 8, None, None, None, _lib.stream()) == ERR_ARG
