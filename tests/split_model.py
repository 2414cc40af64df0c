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


F16_MIN_NORMAL = 2.0 ** -14


def _unnormalised(h):
    """|h| as a rounding of the f16 matrix core sees it: a non-zero subnormal half counts as 2^-14.  v_mfma_f32_*_f16 does
    not normalise a subnormal operand m 2^-24 = (m 2^-10) 2^-14: it adds the product in an fp32-wide window below
    2^-14 |w|, so the rounding of that addition is 2^-24 of 2^-14 |w|, not of |a| |w| -- a half with z leading zeros gives a
    product of 24 - z significant bits (a = 2^-24: 14 bits; a >= 2^-15: exact, the product has 23 bits at most)"""
    a = np.abs(_f64(h))
    return np.where((a > 0) & (a < F16_MIN_NORMAL), F16_MIN_NORMAL, a)


def _mag_unnormalised(ah, al, wh, wl):
    return (_unnormalised(ah) + _unnormalised(al)) @ (_unnormalised(wh) + _unnormalised(wl))


def _clean(a):
    """(a with non-finite-after-split elements replaced by 0, per-row flag: the row holds such an element).  An element
    >= 65520 splits into hi = +inf, lo = -inf (an infinity into inf, NaN; a NaN into NaN, NaN): whatever the weight, the
    three products of such an element sum to NaN (inf * 0 = NaN, inf - inf = NaN), so every output that reads the row is
    NaN in EVERY column.  The model states that directly instead of relying on how a BLAS treats inf * 0."""
    a = np.asarray(a, dtype=np.float32)
    bad = ~np.isfinite(join(*split(a)))
    return np.where(bad, np.float32(0), a), bad.any(axis=-1)


def gemm_model(a, w, flush=False, terms=(1, 1, 1), unnormalised=False):
    """a [M, K] fp32, w [N, K] fp32 (nn.Linear layout) -> (y float64 [M, N], S float64 [M, N], n int [M, 1]).
    unnormalised: S counts subnormal halves as 2^-14 (_unnormalised)"""
    a, bad = _clean(a)
    ah, al = split(a, flush)
    wh, wl, sw = split_weight(np.asarray(w, dtype=np.float32).T, flush)
    y = np.ldexp(_three(ah, al, wh, wl, terms), -sw)
    S = np.ldexp((_mag_unnormalised if unnormalised else _mag)(ah, al, wh, wl), -sw)
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


# ------------------------------------------------------------------------------------------------ the backward
# A backward call multiplies the WHOLE gradient tensor by one power of two s (grad_split_kernel / grad_scale_kernel) and
# its last pass multiplies the result by 1 / s.  Both multiplications are exact (a power of two changes the exponent
# only) unless a result is an fp32 subnormal: the tests keep their values out of that range, except the conversion case
# that scales the tensor by 2^-140 to reach the clamped scale.  Between the two sits the split arithmetic of the forward
# pass on g * s, so the models below are the forward models on g * s, divided by s, and so are the bounds:
#     |dX - model| <= (3 n 2^-24 S + max(2^-22 |y|, 2^-25)) / s        (y = the scaled result the kernel stores as split rows)
#     |dW - model| <=  3 n 2^-24 S / s                                  (fp32 partial blocks, no split store)
# A row that is 2^-k of the tensor's maximum therefore carries an ABSOLUTE error of 2^-25 / s per element from k = 13 on
# (its lo half is an f16 subnormal), loses half its bits at k = 24 and is gone at k = 35: backward_accuracy_table().
GRAD_TOP = np.float32(3.0e38)          # grad_absmax_kernel: |g| <= 3.0e38 sets the scale, larger / inf / NaN pass through it


def grad_scale(g):
    """s of grad_split_kernel / grad_scale_kernel: 2^min(10 - e, 126) with frexp(m) = (f, e), m = the largest |g| that is
    <= 3.0e38 (m * s in [2^9, 2^10)); 1 when no such entry is non-zero.  The clamp keeps s finite for a denormal m."""
    a = np.abs(np.asarray(g, dtype=np.float32)).ravel()
    with np.errstate(invalid="ignore"):
        a = a[a <= GRAD_TOP]
    m = np.float32(a.max()) if a.size else np.float32(0)
    if not m > 0:
        return 1.0
    return 2.0 ** min(10 - int(np.frexp(m)[1]), 126)


def scaled(g, s):
    """g * s as the kernels form it: one fp32 multiplication"""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(g, dtype=np.float32) * np.float32(s)).astype(np.float32)


def pairs_from_nbr(nbr):
    """the pair lists of isf_rulebook_pair_lists from an output-stationary table nbr [K, num_out]: per tap the present
    (input row, output row) pairs in output order -> (pairs_in, pairs_out int [K, max count], -1 padded; counts [K])"""
    nbr = np.asarray(nbr)
    K = nbr.shape[0]
    counts = (nbr >= 0).sum(1)
    pin = np.full((K, max(int(counts.max()), 1)), -1, np.int64)
    pout = pin.copy()
    for k in range(K):
        o = np.flatnonzero(nbr[k] >= 0)
        pin[k, :o.size], pout[k, :o.size] = nbr[k, o], o
    return pin, pout, counts


def transpose_nbr(nbr, num_in):
    """nbr_t [K, num_in]: the output row that tap k of input row i feeds (isf_transpose_rulebook), -1 when none"""
    nbr = np.asarray(nbr)
    out = np.full((nbr.shape[0], num_in), -1, np.int64)
    for k in range(nbr.shape[0]):
        o = np.flatnonzero(nbr[k] >= 0)
        out[k, nbr[k, o]] = o
    return out


def _bad(a):
    """per element: the halves of a are not finite (see _clean)"""
    return ~np.isfinite(join(*split(np.asarray(a, dtype=np.float32))))


def wgrad_model(x, g, pairs_in, pairs_out, counts, flush=False, terms=(1, 1, 1), s=None, unscale=None):
    """dW of wgrad16_kernel: x [N_in, Cin], g [N_out, Cout] fp32, pair lists as pairs_from_nbr -> (dW, S float64
    [K, Cin, Cout], n int [K, 1, 1]: the tap's pair count).  Per tap  sum_p x_lo*g_hi + x_hi*g_lo + x_hi*g_hi  over the
    tap's pairs from the halves of x and of g * s, in float64, times 1 / s; S the same over absolute halves.  There is no
    weight scale.  An element of g (of x) whose halves are not finite makes its COLUMN (row) of every tap that pairs its
    row NaN, and nothing else: inf * 0 = NaN, inf - inf = NaN, whatever the other operand holds.
    The failures the tests must see: flush = True / "g" / "x" (both / one operand's halves lose f16 subnormals), terms,
    s (a scale that grad_scale would not give), unscale (per tap, the factor its sum is multiplied by instead of 1 / s)."""
    s = grad_scale(g) if s is None else s
    gsc = scaled(g, s)
    bx, bg = _bad(x), _bad(gsc)
    xh, xl = split(np.where(bx, np.float32(0), np.asarray(x, dtype=np.float32)), flush in (True, "x"))
    gh, gl = split(np.where(bg, np.float32(0), gsc), flush in (True, "g"))
    K = len(counts)
    dw = np.zeros((K, xh.shape[1], gh.shape[1]), np.float64)
    S = np.zeros_like(dw)
    poisoned = np.zeros(dw.shape, bool)
    for k in range(K):
        i, o = pairs_in[k, :counts[k]], pairs_out[k, :counts[k]]
        if i.size == 0:
            continue
        dw[k] = _three(xh[i].T, xl[i].T, gh[o], gl[o], terms)
        S[k] = _mag(xh[i].T, xl[i].T, gh[o], gl[o])
        poisoned[k] = bx[i].any(0)[:, None] | bg[o].any(0)[None, :]
    inv = np.full(K, 1.0 / s) if unscale is None else np.asarray(unscale, dtype=np.float64)
    dw, S = dw * inv[:, None, None], S / s
    dw[poisoned] = np.nan
    S[poisoned] = np.nan
    return dw, S, np.asarray(counts, dtype=np.int64).reshape(K, 1, 1)


def wgrad_bound(S, n):
    """fp32 partial blocks added in fp32: the accumulation bound alone (S is already divided by s)"""
    return accumulation_bound(S, n)


def dgrad_model(g, w, nbr_t, num_in, flush=False, terms=(1, 1, 1), s=None):
    """dX of a conv with filters w [K, Cin, Cout]: the forward kernel on the split rows of g * s over the transposed table
    with the per-tap transposed filters (one power-of-two scale for the whole filter, as split_weight gives it), its
    split-stored result read back times 1 / s -> (dX float64 [num_in, Cin], bound): conv_model(g s, w_t, nbr_t) / s and
    (3 n 2^-24 S + split_bound(y)) / s."""
    s = grad_scale(g) if s is None else s
    wt = np.ascontiguousarray(np.asarray(w, dtype=np.float32).transpose(0, 2, 1))
    y, S, n = conv_model(scaled(g, s), wt, nbr_t, num_in, flush, terms)
    return y / s, (accumulation_bound(S, n) + split_bound(y)) / s


def linear_dgrad_model(g, w, flush=False, terms=(1, 1, 1), s=None):
    """dX = G W of a Linear with weight w [N, K] (fusion_train.LinearFunction: isf_grad_rescale, the forward GEMM on the
    transposed packed weight, fp32 rows times 1 / s) -> (dX float64 [M, K], bound = 3 n 2^-24 S' / s).
    S' counts a subnormal half as 2^-14 (_unnormalised).  This output has no split store whose 2^-25 would cover its
    small rows, and n is small, so here -- and only here -- the plain S is not met on the GPU: a row at 2^-33 of the
    tensor's maximum (g s ~ 2^-24: one significant bit, 10 leading zeros) comes back 2^-14 (relative) off the model at
    n = 128, against 3 n 2^-24 = 2^-15.4 (worst error / bound = 2.4 for class Grow at 1000 x 128 -> 384; 0.9 at n = 256).
    The error is 1e-5 of what the format itself has already lost of such a row (backward_accuracy_table: 30 % .. 100 %)."""
    s = grad_scale(g) if s is None else s
    y, S, n = gemm_model(scaled(g, s), np.ascontiguousarray(np.asarray(w, dtype=np.float32).T), flush, terms, unnormalised=True)
    return y / s, accumulation_bound(S, n) / s


def rows_wgrad_model(g, x, flush=False, terms=(1, 1, 1), s=None, unscale=None):
    """dW [N, K] = G^T X / s of isf_rows_weight_grad: g [R, N] arrives multiplied by s (isf_grad_rescale), x [R, K] as it
    is; the kernel splits BOTH itself, neither with a weight scale: g_lo*x_hi + g_hi*x_lo + g_hi*x_hi over the R rows
    -> (dW float64, bound = 3 R 2^-24 S / s).  unscale: the factor used instead of 1 / s (scalar)."""
    s = grad_scale(g) if s is None else s
    gh, gl = split(scaled(g, s), flush in (True, "g"))
    xh, xl = split(x, flush in (True, "x"))
    inv = 1.0 / s if unscale is None else unscale
    with np.errstate(invalid="ignore", over="ignore"):          # a wrong scale (the tests try one) overflows the halves
        dw = _three(gh.T, gl.T, xh, xl, terms) * inv
        return dw, accumulation_bound(_mag(gh.T, gl.T, xh, xl), g.shape[0]) / s


# gradient classes: one planted element of 600 (in [2^9, 2^10)) is the tensor's maximum, so s = 1; rows relative to it
GRAD_CLASSES = ("Guni", "Grow", "Gspike", "Gelem", "Gedge")
GRAD_PEAK = np.float32(600.0)
# the edge values a scaled gradient can hold (below 2^9), and the hi ties of the top binade [2^9, 2^10): f16 step 0.5
GRAD_EDGE_VALUES = np.concatenate([[v for v in
                                    (0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 2.0 ** -127, -(2.0 ** -130), 2.0 ** -25,
                                     -(2.0 ** -25), 1.5 * 2.0 ** -24, -1.5 * 2.0 ** -24, 2.0 ** -24, -(2.0 ** -24),
                                     2.5 * 2.0 ** -24, 2.0 ** -26, 2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -14, -(2.0 ** -14),
                                     2.0 ** -14 - 2.0 ** -25, 2.0 ** -14 - 2.0 ** -26, 1 + 2.0 ** -11, -(1 + 2.0 ** -11),
                                     1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -11 - 2.0 ** -23,
                                     0.125 + 2.0 ** -14, 0.125 - 2.0 ** -15, 1 + 2.0 ** -12 + 2.0 ** -23, 1 + 2.0 ** -22,
                                     1 + 3 * 2.0 ** -23, 1.0, -1.0, 0.1, -0.3333333, 1e-3, 1e-5, 1e-7, 3.14159265)],
                                   [512.25, -512.75, 511.99997, 1023.75]]).astype(np.float32)


def make_grad(name, shape, seed, peak_row=None):
    """seeded fp32 gradient rows [rows, cols] of a class (GRAD_CLASSES) -> g with grad_scale(g) == 1:
      Guni    every row O(max): N(0, 1) * 128, clipped to +-500
      Grow    row r times 2^-(r mod 35): lo subnormal from k = 13, hi subnormal from 24, gone at 35 (k = 0 .. 34)
      Gspike  one element at the maximum, everything else 2^-24 of it (N(0, 1) * 2^-15; 2^-15 = 2^9 2^-24)
      Gelem   per-element exponents 2^-(0 .. 34)
      Gedge   GRAD_EDGE_VALUES (every value at least once); its maximum 1023.75 is the peak
    the peak sits in row peak_row (default: a seeded row with k = 0)."""
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    rows, cols = shape
    base = np.clip(rng.standard_normal(shape) * 128.0, -500.0, 500.0)
    if name == "Guni":
        g = base
    elif name == "Grow":
        g = base * np.exp2(-(np.arange(rows) % 35.0))[:, None]
    elif name == "Gspike":
        g = base * 2.0 ** -22
    elif name == "Gelem":
        g = base * np.exp2(-rng.integers(0, 35, shape).astype(np.float64))
    elif name == "Gedge":
        g = GRAD_EDGE_VALUES[rng.integers(0, GRAD_EDGE_VALUES.size - 1, shape)].astype(np.float64)
        g.reshape(-1)[:GRAD_EDGE_VALUES.size - 1] = GRAD_EDGE_VALUES[:-1]
    else:
        raise ValueError(name)
    g = g.astype(np.float32)
    r = (35 * int(rng.integers(1, max(rows // 35, 2))) if rows > 70 else 0) if peak_row is None else peak_row
    g[r, int(rng.integers(0, cols))] = GRAD_EDGE_VALUES[-1] if name == "Gedge" else GRAD_PEAK
    assert grad_scale(g) == 1.0
    return g


# what the non-finite tests plant: an infinity, a NaN, and a FINITE value above 3.0e38 -- it does not set the scale
# either and overflows f16 once it is split
GRAD_POISON = np.array([np.inf, np.nan, 3.2e38], dtype=np.float32)


def backward_accuracy_table(seed=0, n=256, rows=64, outs=64):
    """(k, relative error of dX, relative error of dW) of a gradient row at 2^-k of the tensor's maximum: model against
    the exact float64 product of the same fp32 operands, each relative to that row's own exact contribution.  A Linear
    with n inputs, `rows` gradient rows of N(0, 1) * 128 times 2^-k next to one row at the maximum (600), O(1)
    activations; dW is the row's contribution g_r^T x_r alone.  The table quoted by DESIGN.md section 6 / INTEGRATION.md
    section 4."""
    rng = np.random.default_rng(seed)
    w = rng.normal(0, (1.0 / n) ** 0.5, (outs, n)).astype(np.float32)
    base = np.clip(rng.standard_normal((rows, outs)) * 128.0, -500, 500)
    x = rng.standard_normal((rows, n)).astype(np.float32)
    out = []
    for k in (0, 6, 12, 13, 16, 20, 24, 28, 32, 34, 35, 40):
        g = (base * 2.0 ** -k).astype(np.float32)
        g[0, :] = 0
        g[0, 0] = GRAD_PEAK
        dx, _ = linear_dgrad_model(g, w)
        ex = g.astype(np.float64) @ w.astype(np.float64)
        r = 1 + int(np.argmax(np.abs(ex[1:]).max(1)))
        one = np.zeros_like(g)
        one[r] = g[r]
        dw, _ = rows_wgrad_model(one, x, s=grad_scale(g))
        ew = one.astype(np.float64).T @ x.astype(np.float64)
        out.append((k, float(np.abs(dx[1:] - ex[1:]).max() / np.abs(ex[1:]).max()),
                    float(np.abs(dw - ew).max() / np.abs(ew).max())))
    return out


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
