"""The yardstick of the cross-rank exact sums (isfusion_amd.collectives, csrc/isf_fixed_reduce.hip): a big-integer model
of pack, sum and finish, and the recipes the CPU and GPU tests share.

The model restates the kernels' arithmetic, not their code: numpy's rint has llrint's ties-to-even, Python ints hold the
packed values and their sums (no width to overflow), and the finish goes the kernels' way -- the integer to a double
(Python's int -> float rounds to nearest even, as the conversion instruction does), an exact scaling, one double division
and one rounding to float32."""
import itertools
from fractions import Fraction

import numpy as np

INF_BITS = 0x7f800000


def ceil_log2(n):
    return max(int(n) - 1, 0).bit_length()


def abs_bits(x):
    """bit patterns of |x| (uint32), the quantity the bound is an integer maximum of"""
    return np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0x7fffffff)


def bound_bits(*contribs):
    """the bound of one tensor: the largest pattern of |x| over every contribution (0 for no elements)"""
    return max((int(abs_bits(c).max()) for c in contribs if np.size(c)), default=0)


def exponent(bits, log2n):
    """e = 62 - log2n - ex, A < 2^ex; None when the bound is an inf or a NaN"""
    if bits >= INF_BITS:
        return None
    ex = int(np.frexp(np.array([bits], np.uint32).view(np.float32)[0])[1])
    return 62 - log2n - ex


def pack(x, e):
    """[int]: llrint(x * 2^e) per element (e None: zeros)"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    if e is None:
        return [0] * x.size
    return [int(v) for v in np.rint(np.ldexp(x.astype(np.float64), e))]


def finish(sums, e, divisor, n=None):
    """float32 [n]: float(double(S) * 2^-e / divisor); NaN everywhere when e is None"""
    if e is None:
        return np.full(len(sums) if n is None else n, np.nan, np.float32)
    d = np.array([float(s) for s in sums], np.float64)
    return (np.ldexp(d, -e) / np.float64(divisor)).astype(np.float32)


def reduce_tensor(contribs, divisor, log2n=None):
    """one tensor over its W contributions (the gradient path): one bound for the whole tensor.  -> (bits, e, sums, out)"""
    log2n = ceil_log2(len(contribs)) if log2n is None else log2n
    bits = bound_bits(*contribs)
    e = exponent(bits, log2n)
    sums = [sum(col) for col in zip(*[pack(c, e) for c in contribs])]
    return bits, e, sums, finish(sums, e, divisor)


def sum_rows(rows, divisor=1.0):
    """isf_fixed_sum_rows: every column has its own bound"""
    rows = np.ascontiguousarray(rows, np.float32)
    w, n = rows.shape
    es = [exponent(int(b), ceil_log2(w)) for b in abs_bits(rows).max(axis=0)]
    finite = np.array([e is not None for e in es])
    q = np.rint(np.ldexp(np.where(finite, rows, 0).astype(np.float64), np.array([e or 0 for e in es])))
    out = np.empty(n, np.float32)
    for c in range(n):
        out[c] = finish([sum(int(v) for v in q[:, c])], es[c], divisor)[0]
    return out


def exact_mean(contribs, divisor):
    """[Fraction]: the rational sum of the contributions / divisor"""
    cols = zip(*[[Fraction(float(v)) for v in np.asarray(c, np.float32).reshape(-1)] for c in contribs])
    return [sum(col) / Fraction(divisor) for col in cols]


def ulp32(v):
    """the spacing of float32 at |v| (the subnormal spacing below the normal range)"""
    v = abs(float(v))
    if v == 0.0:
        return 2.0 ** -149
    return 2.0 ** (max(int(np.floor(np.log2(v))), -126) - 23)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------------ recipes
def mixed(rs, shape):
    """magnitudes spread over 2^-20 .. 2^0: the sequential fp32 sum of such rows depends on their order"""
    return (rs.normal(size=shape) * 2.0 ** rs.randint(-20, 1, size=shape)).astype(np.float32)


def rank_recipe(world=4, n=4096, seed=7):
    return mixed(np.random.RandomState(seed), (world, n))


def cancelling_recipe(n=1024, seed=11):
    """x, -x and a tiny third row: the float sum keeps the tiny row only in the order that cancels first"""
    rs = np.random.RandomState(seed)
    x = rs.normal(size=n).astype(np.float32)
    tiny = (rs.normal(size=n) * 2.0 ** -30).astype(np.float32)
    return np.stack([x, -x, tiny])


def sequential_sum(rows, order):
    """the float32 sum a ring would form: one rounding per add, in `order`"""
    s = np.zeros(rows.shape[1], np.float32)
    for r in order:
        s = (s + rows[r]).astype(np.float32)
    return s


def orders(world):
    return list(itertools.permutations(range(world)))


COUNTS = (1, 3, 513, 4097, 32768 + 1)            # ISF_OPTIM_CHUNK + 1: a second chunk of one element
KINDS = ("tiny", "unit", "mixed", "zero", "nan", "inf")


def tensor_of(kind, n, rs):
    if kind == "tiny":
        return (rs.normal(size=n) * 1e-9).astype(np.float32)
    if kind == "unit":
        return rs.normal(size=n).astype(np.float32)
    if kind == "zero":
        return np.zeros(n, np.float32)
    x = mixed(rs, n)
    if kind == "nan":
        x[n // 2] = np.nan
    if kind == "inf":
        x[n - 1] = -np.inf
    return x


def parse_data_order(text, world):
    """--data-order of tools/train_step.py: 'i,j,k' -> [i, j, k], a permutation of range(world); '' -> the identity"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "train_step.py")
    spec = importlib.util.spec_from_file_location("_train_step_cli", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.parse_data_order(text, world)
