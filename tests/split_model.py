"""Float64 reference model of the "f16x3" split arithmetic (numpy only, no GPU).

Every matrix-core kernel of the forward path carries an fp32 operand x as two f16 halves,

    hi = f16(x)            lo = f16(x - hi)            (round to nearest even, subnormals kept)

and evaluates a product as  a_lo*b_hi + a_hi*b_lo + a_hi*b_hi  with fp32 accumulation.  Weights are multiplied by a power
of two 2^sw with max|w| * 2^sw in [2^12, 2^13) before they are split (pack_filters16_kernel, isf_pack_linear) and the
result is multiplied by 2^-sw; activations are not scaled.

The model evaluates the SAME three products from the SAME halves, but sums them in float64: an f16 x f16 product has 22
significant bits, so float64 sums of a few thousand of them are exact to ~2^-40 relative -- far below the fp32
accumulation error the tests allow.  What a kernel may differ by is therefore only the order and rounding of its fp32
accumulation, bounded per output element by

    |y_kernel - y_model| <= 3 n 2^-24 S,      S = sum_k (|a_hi| + |a_lo|)(|w_hi| + |w_lo|) 2^-sw      (n products of a row)

(3 n exact products, at most 3 n - 1 roundings of partial sums each bounded by u * sum|terms| <= 2^-24 S).
A kernel that flushes f16 subnormals, truncates, or drops a term leaves this bound by orders of magnitude
(tests/test_split_model.py proves that on the CPU).
"""
import numpy as np

F16_MAX = 65504.0
U32 = 2.0 ** -24          # unit roundoff of fp32
CLASSES = ("A", "B", "C", "D", "E_row", "E_elem", "F")     # finite classes; "G" = overflow, planted in class C


# ------------------------------------------------------------------------------------------------ the format
def _flush(h):
    """f16 array with its subnormal values replaced by (signed) zero -- the FAILURE the tests must be able to see"""
    h = h.copy()
    sub = (np.abs(h) < np.float16(2.0 ** -14)) & (h != 0)
    h[sub] = np.copysign(np.float16(0), h[sub])
    return h


def split(x, flush=False):
    """fp32 -> (hi, lo) float16, exactly split8 of isf_spconv16.h.  flush=True: the broken variant that loses f16
    subnormals."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16)
        if flush:
            hi = _flush(hi)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
        if flush:
            lo = _flush(lo)
    return hi, lo


def join(hi, lo):
    """hi + lo in fp32 (join8)"""
    with np.errstate(invalid="ignore"):
        return hi.astype(np.float32) + lo.astype(np.float32)


def store_split(y):
    """what a kernel that writes split rows returns for the fp32 value y"""
    return join(*split(np.asarray(y, dtype=np.float32)))


def split_bound(x):
    """|join(split(x)) - x| <= max(2^-22 |x|, 2^-25): 22 significant bits while lo is a normal f16 number, half an f16
    subnormal step below"""
    return np.maximum(2.0 ** -22 * np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -25)


def weight_scale(w):
    """sw with max|w| * 2^sw in [2^12, 2^13) (0 for an all-zero weight): `sw = 13 - e`, frexp(max|w|) = (m, e)"""
    amax = float(np.abs(np.asarray(w, dtype=np.float32)).max()) if np.size(w) else 0.0
    if not amax > 0.0:
        return 0
    return 13 - int(np.frexp(np.float32(amax))[1])


def split_weight(w, flush=False):
    """-> (w_hi, w_lo, sw): halves of w * 2^sw"""
    sw = weight_scale(w)
    ws = np.ldexp(np.asarray(w, dtype=np.float32), sw).astype(np.float32)
    hi, lo = split(ws, flush)
    return hi, lo, sw


def to_split_bytes(x):
    """the split activation buffer of x [N, C] (C % 32 == 0) as uint16 [N * C / 32, 2, 32]: per 32-channel chunk the 32 hi
    halves, then the 32 lo halves (isf_common.h, "split activation format")"""
    hi, lo = split(x)
    n = hi.size // 32
    return np.stack([hi.reshape(n, 32).view(np.uint16), lo.reshape(n, 32).view(np.uint16)], 1)


# ------------------------------------------------------------------------------------------------ the products
def _f64(h):
    return h.astype(np.float64)


def _three(ah, al, wh, wl, terms=(1, 1, 1)):
    """a_lo*w_hi, a_hi*w_lo, a_hi*w_hi summed in float64; a [M, K], w [K, N] halves (finite).  terms: which of the three
    products to keep (the tests switch one off to prove they would notice)"""
    y = np.zeros((ah.shape[0], wh.shape[1]), np.float64)
    if terms[0]:
        y += _f64(al) @ _f64(wh)
    if terms[1]:
        y += _f64(ah) @ _f64(wl)
    if terms[2]:
        y += _f64(ah) @ _f64(wh)
    return y


def _mag(ah, al, wh, wl):
    return (np.abs(_f64(ah)) + np.abs(_f64(al))) @ (np.abs(_f64(wh)) + np.abs(_f64(wl)))


def _clean(a):
    """(a with non-finite-after-split elements replaced by 0, per-row flag: the row holds such an element).  An element
    >= 65520 splits into hi = +inf, lo = -inf (an infinity into inf, NaN; a NaN into NaN, NaN): whatever the weight, the
    three products of such an element sum to NaN (inf * 0 = NaN, inf - inf = NaN), so every output that reads the row is
    NaN in EVERY column.  The model states that directly instead of relying on how a BLAS treats inf * 0."""
    a = np.asarray(a, dtype=np.float32)
    bad = ~np.isfinite(join(*split(a)))
    return np.where(bad, np.float32(0), a), bad.any(axis=-1)


def gemm_model(a, w, flush=False, terms=(1, 1, 1)):
    """a [M, K] fp32, w [N, K] fp32 (nn.Linear layout) -> (y float64 [M, N], S float64 [M, N], n int [M, 1])"""
    a, bad = _clean(a)
    ah, al = split(a, flush)
    wh, wl, sw = split_weight(np.asarray(w, dtype=np.float32).T, flush)
    y = np.ldexp(_three(ah, al, wh, wl, terms), -sw)
    S = np.ldexp(_mag(ah, al, wh, wl), -sw)
    y[bad] = np.nan
    S[bad] = np.nan
    return y, S, np.full((a.shape[0], 1), a.shape[1], np.int64)


def conv_model(feats, w, nbr, num_out, flush=False, terms=(1, 1, 1)):
    """feats [N_in, Cin] fp32, w [K, Cin, Cout] fp32 (one power-of-two scale for the whole filter), nbr int [K, >= num_out]
    (output-stationary: input row of tap k of output o, < 0 when absent) -> (y, S [num_out, Cout] float64, n [num_out, 1]:
    products of a row = present taps * Cin).  Absent taps add exact zeros: they cost no rounding."""
    feats, bad = _clean(feats)
    w = np.asarray(w, dtype=np.float32)
    K, cin, cout = w.shape
    ah, al = split(feats, flush)
    wh, wl, sw = split_weight(w, flush)
    y = np.zeros((num_out, cout), np.float64)
    S = np.zeros((num_out, cout), np.float64)
    n = np.zeros((num_out, 1), np.int64)
    poisoned = np.zeros(num_out, bool)
    for k in range(K):
        idx = np.asarray(nbr[k, :num_out])
        m = idx >= 0
        if not m.any():
            continue
        src = idx[m]
        y[m] += _three(ah[src], al[src], wh[k], wl[k], terms)
        S[m] += _mag(ah[src], al[src], wh[k], wl[k])
        n[m, 0] += cin
        poisoned[m] |= bad[src]
    y, S = np.ldexp(y, -sw), np.ldexp(S, -sw)
    y[poisoned] = np.nan
    S[poisoned] = np.nan
    return y, S, n


def accumulation_bound(S, n):
    """3 n 2^-24 S: the worst fp32 accumulation error of 3 n exact products, in any order"""
    return 3.0 * np.maximum(n, 1) * U32 * S


def gemm_fp32_sequential(a, w, flush=False):
    """the three-product sum accumulated term by term in fp32 (one of the orders a kernel may use) -> fp32 [M, N]"""
    ah, al = split(np.asarray(a, dtype=np.float32), flush)
    wh, wl, sw = split_weight(np.asarray(w, dtype=np.float32).T, flush)
    f = lambda h: h.astype(np.float32)
    acc = np.zeros((ah.shape[0], wh.shape[1]), np.float32)
    for k in range(ah.shape[1]):
        acc = acc + f(al[:, k, None]) * f(wh[None, k, :])
        acc = acc + f(ah[:, k, None]) * f(wl[None, k, :])
        acc = acc + f(ah[:, k, None]) * f(wh[None, k, :])
    return np.ldexp(acc, -sw).astype(np.float32)


# ------------------------------------------------------------------------------------------------ operand classes
CLASS_SCALE = {"A": 2.0 ** -17, "B": 2.0 ** -9, "C": 1.0, "D": 2.0 ** 12}
CLIP = 6.0e4

EDGE_VALUES = np.array(
    [0.0, -0.0,
     1e-45, -1e-45, 1e-40, -1e-40, 2.0 ** -127, -(2.0 ** -130),                 # fp32 subnormals
     2.0 ** -25, -(2.0 ** -25), 1.5 * 2.0 ** -24, -1.5 * 2.0 ** -24,            # ties on the f16 subnormal grid
     2.0 ** -24, -(2.0 ** -24), 2.5 * 2.0 ** -24, 2.0 ** -26, 2.0 ** -25 * (1 + 2.0 ** -20),
     2.0 ** -14, -(2.0 ** -14), 2.0 ** -14 - 2.0 ** -25, 2.0 ** -14 - 2.0 ** -26,   # the normal / subnormal border
     1 + 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -11 - 2.0 ** -23,   # hi ties
     2049.0, 2051.0, 0.125 + 2.0 ** -14, 0.125 - 2.0 ** -15,                   # hi ties; lo at the border of normal
     1 + 2.0 ** -12 + 2.0 ** -23, 1 + 2.0 ** -22, 1 + 3 * 2.0 ** -23,            # lo ties
     1.0, -1.0, 0.1, -0.3333333, 1e-3, 1e-5, 1e-7, 3.14159265, 1234.5677,
     65504.0, -65504.0, 65519.9, -65519.9, 65503.99, 32768.0 + 15.99],
    dtype=np.float32)

OVERFLOW_VALUES = np.array([65520.0, -65520.0, 65536.0, 7.0e4, -1.0e5, 3.0e38, np.inf, -np.inf, np.nan], dtype=np.float32)


def make_class(name, shape, seed):
    """seeded fp32 operands [rows, cols] of a magnitude class (see CLASSES); all scales are powers of two"""
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    rows, cols = shape
    x = rng.standard_normal(shape)
    if name in CLASS_SCALE:
        x = x * CLASS_SCALE[name]
    elif name == "E_row":
        x = x * np.exp2(rng.integers(-20, 14, (rows, 1)))
    elif name == "E_elem":
        x = x * np.exp2(rng.integers(-20, 14, shape))
    elif name == "F":
        x = EDGE_VALUES[rng.integers(0, EDGE_VALUES.size, shape)].astype(np.float64)
        x.reshape(-1)[:EDGE_VALUES.size] = EDGE_VALUES[:x.size]       # every edge value at least once
    else:
        raise ValueError(name)
    return np.clip(x, -CLIP, CLIP).astype(np.float32) if name != "F" else x.astype(np.float32)


def make_overflow(shape, seed, rows=6):
    """class G: class-C data with the overflow values planted, one per row, in `rows`-ish distinct rows -> (x, poisoned
    row indices)"""
    rng = np.random.default_rng([seed, 71])
    x = make_class("C", shape, seed)
    pr = np.sort(rng.choice(shape[0], max(rows, OVERFLOW_VALUES.size), replace=False))
    for i, r in enumerate(pr):
        x[r, rng.integers(0, shape[1])] = OVERFLOW_VALUES[i % OVERFLOW_VALUES.size]
    return x, pr


def accuracy_table(seed=0, n=576, outs=64, rows=256):
    """(max|a|, max|model - exact| / max|exact|) per activation scale: N(0,1) * s activations, conv-like weights
    N(0, 1/n), an n-term dot product.  The table quoted by DESIGN.md section 6 / INTEGRATION.md section 4."""
    rng = np.random.default_rng(seed)
    w = rng.normal(0, (1.0 / n) ** 0.5, (outs, n)).astype(np.float32)
    base = rng.standard_normal((rows, n))
    out = []
    for e in (0, -3, -7, -10, -13, -14, -17, -20):
        a = (base * 2.0 ** e).astype(np.float32)
        exact = a.astype(np.float64) @ w.astype(np.float64).T
        y, _, _ = gemm_model(a, w)
        out.append((float(np.abs(a).max()), float(np.abs(y - exact).max() / np.abs(exact).max())))
    a = base.astype(np.float32)
    a[0, 0] = 65520.0
    y, _, _ = gemm_model(a, w)
    out.append((65520.0, float(y[0, 0])))
    return out
