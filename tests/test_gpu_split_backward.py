"""The split-precision kernels of the BACKWARD pass, per element, at every gradient magnitude (-m gpu).

A backward call multiplies the whole gradient tensor by ONE power of two s that brings max|g| into [2^9, 2^10)
(isf_grad_to_split / isf_grad_rescale), runs the forward's f16x3 arithmetic on g * s and multiplies the result by 1 / s.
A gradient row that is small against the tensor's largest element -- the normal state of a backward pass -- therefore
sits in f16 subnormals, first with its lo half (2^-13 of the maximum), then with its hi half (2^-24), and is gone at
2^-35.  The rest of the GPU tier divides errors by the tensor's maximum and uses uniform scales, which cancel exactly: a
flushed subnormal, a lost lo product, a tail masked on one side, an inverse scale applied twice to one chunk are 1e-3 of
the maximum or less, and up to 100 % of a small row.  Here every result is judged per element against
tests/split_model.py (wgrad_model, dgrad_model, linear_dgrad_model, rows_wgrad_model: the same halves of g * s, the same
products, summed in float64, times 1 / s) on gradient classes built so that a planted element of 600 makes s = 1:

    Guni   every row O(max)            Grow  row r at 2^-(r mod 35) of the maximum       Gspike  one element, the rest 2^-24
    Gelem  per-element exponents       Gedge edge values (ties, the subnormal border, fp32 subnormals)

with activations of the forward tier's classes A-E (split_backward_cases.PAIRS):
  (a) the conversion kernels, bit for bit, the clamped scale, zero and non-finite tensors included;
  (b) selection probes: filters of single 1.0 entries (dX) and unit-vector activation rows (dW) make every product and
      sum exact, so the result must EQUAL the selected gradient halves -- conversions, gathers, tail masking and the
      inverse scale observed exactly;
  (c) random operands: |got - model| <= 3 n 2^-24 S / s (+ the split store of dX, max(2^-22 |y|, 2^-25) / s); for
      LinearFunction's dX, S counts a subnormal half as 2^-14 (split_model.linear_dgrad_model says why and what was measured);
  (d) scale equivariance: the gradient times 2^-40 / 2^30 gives the same bits times that power of two;
  (e) non-finite gradients are loud and confined to the dX rows and dW columns that pair their row.
tests/test_split_model.py shows on these inputs that each bound is met by an honest fp32 evaluation and left by each of
seven defects.  Each check prints one line `split-domain bwd <family> <class>: ...` (run with -s)."""
import numpy as np
import pytest
import torch

import split_backward_cases as sc
import split_model as sm
from test_gpu_split_domain import T, check_bound, check_equal, selected, selection_weight
from isfusion_amd import _lib

pytestmark = pytest.mark.gpu


def report_equal(family, cls, what):
    print(f"split-domain bwd {family} {cls}: equal ({what})")


def is_nan16(bits):
    return (bits & 0x7FFF) > 0x7C00


def same_f32(got, want):
    """fp32 arrays equal bit for bit; NaNs compared as NaNs (IEEE leaves their sign and payload open)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


# ------------------------------------------------------------------------------------------------ (a) conversions
def conversion_cases():
    """(name, g): every class as built (s = 1), times 2^-120 (s = 2^120), times 2^-140 (the maximum 600 2^-140 is an fp32
    subnormal: 10 - e = 141, the clamp gives s = 2^126 and the scaled maximum stays below 2^9), times 2^100 (s = 2^-100);
    zeros; Guni with inf, -inf, NaN and a finite 3.2e38 (none of them sets the scale, all pass through it)"""
    out = []
    for cls in sm.GRAD_CLASSES:
        g = sm.make_grad(cls, (1024, 64), 3)
        out.append((cls, g))
        for e in (-120, -140, 100):
            with np.errstate(under="ignore"):
                out.append((f"{cls} x 2^{e}", (g * np.float32(2.0 ** e)).astype(np.float32)))
    out.append(("zero", np.zeros((1024, 64), np.float32)))
    g = sm.make_grad("Guni", (1024, 64), 4)
    g[5, 7], g[17, 0], g[500, 63], g[1023, 31] = np.inf, -np.inf, np.nan, 3.2e38
    out.append(("non-finite", g))
    return out


def test_gradient_conversions_bit_for_bit(dev):
    """isf_grad_to_split == the BITS of split(g * s) and scale_out == {s, 1 / s}; isf_grad_rescale == g * s;
    isf_split_to_f32_scaled == join(hi, lo) * (1 / s), all with s = split_model.grad_scale(g).  The multiplications by s and
    1 / s are single fp32 operations, so numpy's are the same bits -- also where the result is an fp32 subnormal (the
    2^-140 case, the only one here that reaches that range on the way back)."""
    from isfusion_amd import spconv as sp
    for name, g in conversion_cases():
        s = sm.grad_scale(g)
        if name == "zero":
            assert s == 1.0
        if " x 2^-140" in name:
            assert s == 2.0 ** 126 and 0 < np.abs(g).max() < 2.0 ** -126
        if name == "non-finite":
            assert s == 1.0 and (~np.isfinite(g)).sum() == 3
        gsc = sm.scaled(g, s)
        want = sm.to_split_bytes(gsc)
        gs, scale = sp.grad_to_split(T(g, dev))
        assert scale.cpu().numpy().tolist() == [s, 1.0 / s], (name, scale.cpu().numpy().tolist(), s)
        got = gs.cpu().numpy().view(np.uint16).reshape(want.shape)
        nan = is_nan16(want)
        assert np.array_equal(is_nan16(got), nan) and np.array_equal(got[~nan], want[~nan]), name
        assert name == "non-finite" or not nan.any()
        out, scale2 = _lib.grad_rescale(T(g, dev))
        assert scale2.cpu().numpy().tolist() == [s, 1.0 / s], name
        assert same_f32(out.cpu().numpy(), gsc), name
        with np.errstate(under="ignore", invalid="ignore"):
            back = sm.join(*sm.split(gsc)) * np.float32(1.0 / s)
        assert same_f32(sp.from_split_scaled(gs, g.shape, scale[1:]).cpu().numpy(), back), name
        if name == "zero":
            assert not got.any() and not out.cpu().numpy().any()
        report_equal("grad_to_split / grad_rescale / split_to_f32_scaled", name, f"bits, s = 2^{int(np.log2(s))}")


# ------------------------------------------------------------------------------------------------ conv plumbing
def wgrad_wk(cin, cout):
    """waves that split a workgroup's pair range (wgrad16_shape: 4 / (WM WN))"""
    return 4 // ((2 if cin >= 128 else 1) * (2 if cout >= 128 else 1))


def rulebook(dev, cin, cout, geo):
    """-> (rb, nbr [K, num_out], nbr_t [K, num_in], pair lists, rows): the library's rulebook of the seeded geometry, its
    tables checked against split_model's restatement of the transposition and the pair compaction"""
    from isfusion_amd import spconv as sp
    rows = sc.conv_rows(cin, cout)
    idx = sc.geometry(cin + cout, rows)
    rb = sp.build_rulebook(T(idx, dev), 2, list(sc.GRID), geo[1], geo[2], geo[3], geo[0])
    K = 27
    nbr = np.maximum(rb.nbr.view(K, rb.stride)[:, :rb.num_out].cpu().numpy().astype(np.int64), -1)
    assert rb.num_in == rows
    sc.check_rulebook(nbr, wgrad_wk(cin, cout), chunks3=geo[0])
    nbr_t = sm.transpose_nbr(nbr, rows)
    rbt = rb.transposed()
    assert np.array_equal(np.maximum(rbt.nbr.view(K, rbt.stride)[:, :rows].cpu().numpy(), -1), nbr_t)
    pin, pout, counts = sm.pairs_from_nbr(nbr)
    pairs, num, cap = sp.pair_lists(rb)
    pairs = pairs.cpu().numpy()
    assert np.array_equal(num.cpu().numpy(), counts)
    for k in range(K):
        assert np.array_equal(pairs[k, 0, :counts[k]], pin[k, :counts[k]])
        assert np.array_equal(pairs[k, 1, :counts[k]], pout[k, :counts[k]])
    return rb, nbr, nbr_t, (pin, pout, counts), rows


def run_backward(dev, rb, x, g, w, half=False, want_dx=True, want_dw=True, flags=0):
    """spconv.split_backward as SparseConvFunction.backward calls it -> (dX, dW [K, cin, cout]) numpy"""
    from isfusion_amd import spconv as sp
    K, cin, cout = w.shape
    k3 = (3, 3, 3) if K == 27 else (1, 3, 3)
    xs = sp.to_split(T(x, dev))
    gs, scale = sp.grad_to_split(T(g, dev))
    pt = sp.pack_filters_f16x3(T(w.reshape(*k3, cin, cout), dev), transposed=True)
    dx, dw = sp.split_backward(xs, gs, scale, rb, pt, K, cin, cout, half, want_dx, want_dw, (*k3, cin, cout), flags)
    return (dx.cpu().numpy() if want_dx else None), (dw.view(K, cin, cout).cpu().numpy() if want_dw else None)


HALF_BOUND = 1.0 / 3.0      # single-pass f16: n exact products instead of 3 n -> n 2^-24 S = accumulation_bound / 3


# ------------------------------------------------------------------------------------------------ (b) probes
@pytest.mark.parametrize("cin,cout", sc.CONV_SHAPES)
def test_conv_backward_selection_probes(dev, cin, cout):
    """SubM rulebook, every gradient class, as built (s = 1) and times 2^-40 (s = 2^40: the inverse scale is observed).
    dX  filters of single 1.0 entries (column c of dX takes tap t(c), gradient channel pi(c)): dX == join(split(g s)) / s
        of the selected gradient row, 0 where the transposed table has no entry.
    dW  activation rows that are unit vectors: `cin` rows, one per channel -- the first and the last row, the rows at the
        chunk borders 255 / 256 / 511 / 512 and seeded others, all other rows zero -- so a tap pairs each channel at most
        once and dW[k][ci, :] == join(split(g s)) / s of THAT pair's gradient row (hi + lo is exact in fp32, every other
        product an exact zero), 0 where the tap does not pair the row.  Single-pass f16 mode: the hi half alone.
        The unit is 1.0 and nothing smaller.  A unit of 2^-20 (an f16 subnormal) is NOT exact on the matrix cores: they
        do not normalise a subnormal operand, so its product keeps 24 bits below 2^-14 |g|, not below 2^-20 |g| -- the
        results came back 2^-19 (relative) off, the last bits of hi + lo gone (split_model._unnormalised)."""
    rb, nbr, nbr_t, _, rows = rulebook(dev, cin, cout, sc.SUBM)
    K = 27
    taps = np.flatnonzero((nbr_t >= 0).any(1)).tolist() + [0, 26]                    # the nine taps with pairs, two without
    wt, t, pi = selection_weight(K, cout, cin, cin * 3 + cout, taps)                # [K, cout, cin]: the dX conv's filters
    w = np.ascontiguousarray(wt.transpose(0, 2, 1))
    rng = np.random.default_rng(cin + cout)
    fixed = np.array([0, rows - 1, 255, 256, 511, 512])
    for cls in sm.GRAD_CLASSES:
        for f in (1.0, 2.0 ** -40):
            with np.errstate(under="ignore"):
                g = (sm.make_grad(cls, (rb.num_out, cout), 7) * np.float32(f)).astype(np.float32)
            s = sm.grad_scale(g)
            assert s == 1.0 / f
            gsc = sm.scaled(g, s)
            gj, inv = sm.join(*sm.split(gsc)), np.float32(1.0 / s)
            dx, _ = run_backward(dev, rb, np.zeros((rows, cin), np.float32), g, w, want_dw=False)
            check_equal(f"bwd dX {cin}->{cout} [selection]", cls, dx, selected(gj, nbr_t, t, pi) * inv)
            for _ in range(2):                                                      # two seeded choices of rows
                others = rng.permutation(np.setdiff1d(np.arange(rows), fixed))[:cin - fixed.size]
                chosen = rng.permutation(np.concatenate([fixed, others]))           # chosen[ci]: the row of channel ci
                x = np.zeros((rows, cin), np.float32)
                x[chosen, np.arange(cin)] = 1.0
                o = nbr_t[:, chosen]                                                # [K, cin]: the paired output row
                for half, halves in ((False, gj), (True, sm.split(gsc)[0].astype(np.float32))):
                    want = np.where((o >= 0)[:, :, None], halves[np.maximum(o, 0)], np.float32(0)) * inv
                    _, dw = run_backward(dev, rb, x, g, w, half=half, want_dx=False)
                    check_equal(f"bwd dW {cin}->{cout} [unit rows{', f16' if half else ''}]", cls, dw, want)
        report_equal(f"conv {cin}->{cout} dX [selection], dW [unit rows; f16x3 and f16]", cls,
                     "to the selected gradient halves, s = 1 and 2^40")


# ------------------------------------------------------------------------------------------------ (c) + (d)
def equivariant(family, cls, base, run):
    """(d): the gradient times a power of two gives the SAME bits times that power of two.  run(f) -> results for g * f"""
    for f in sc.FACTORS:
        for name, a, b in zip(("dX", "dW"), base, run(f)):
            if a is not None:
                check_equal(f"bwd {family} {name} [x 2^{int(np.log2(f))}]", cls, b, a * np.float32(f))
    report_equal(family, cls, "bit for bit under 2^-40 and 2^30 on the gradient")


def conv_backward_case(dev, family, rb, nbr_t, lists, x_rows, num_out, w, flags=0, run=None):
    """(c) and (d) of one rulebook: dX per gradient class, dW per (gradient, activation) pair, both arithmetic modes"""
    K, cin, cout = w.shape
    run = run or (lambda x, g, half, want_dx, want_dw: run_backward(dev, rb, x, g, w, half, want_dx, want_dw, flags))
    seen = set()
    for gcls, xcls in sc.PAIRS:
        g = sm.make_grad(gcls, (num_out, cout), 13)
        x = sm.make_class(xcls, (x_rows, cin), 31)
        want_dx = gcls not in seen
        seen.add(gcls)
        dx, dw = run(x, g, False, want_dx, True)
        if want_dx:
            y, bound = sm.dgrad_model(g, w, nbr_t, x_rows)
            assert np.isfinite(y).all() and 0 < np.abs(y).max() < 6e4, gcls
            check_bound(f"bwd {family} dX", gcls, dx, y, bound)
        m, S, n = sm.wgrad_model(x, g, *lists)
        assert np.isfinite(m).all() and np.abs(m).max() > 0
        check_bound(f"bwd {family} dW", f"{gcls} x {xcls}", dw, m, sm.wgrad_bound(S, n))
        if gcls in ("Guni", "Grow"):
            equivariant(family, f"{gcls} x {xcls}", (dx, dw), lambda f: run(x, sc.factor(g, f), False, want_dx, True))
        if (gcls, xcls) in sc.HALF_PAIRS:
            dx, dw = run(x, g, True, True, True)
            y, bound = sm.dgrad_model(g, w, nbr_t, x_rows, terms=(0, 0, 1))
            m, S, n = sm.wgrad_model(x, g, *lists, terms=(0, 0, 1))
            # single pass: n products, not 3 n; the split store of dX is unchanged
            check_bound(f"bwd {family} dX [f16]", gcls, dx, y, sm.split_bound(y) + (bound - sm.split_bound(y)) * HALF_BOUND)
            check_bound(f"bwd {family} dW [f16]", f"{gcls} x {xcls}", dw, m, sm.wgrad_bound(S, n) * HALF_BOUND)
            equivariant(family + " [f16]", f"{gcls} x {xcls}", (dx, dw), lambda f: run(x, sc.factor(g, f), True, True, True))


@pytest.mark.parametrize("geo", [sc.SUBM, sc.STRIDED], ids=["subm", "stride2"])
@pytest.mark.parametrize("cin,cout", sc.CONV_SHAPES)
def test_sparse_conv_backward_componentwise(dev, cin, cout, geo):
    """spconv.split_backward (dX: the forward kernel over the transposed rulebook; dW: wgrad16_kernel) on seeded conv-like
    filters N(0, 1 / (6 cin)): every distinct workgroup shape of wgrad16_shape, a rulebook with taps of zero, ragged and
    (SubM) three-chunk pair counts (split_backward_cases.check_rulebook)."""
    rb, nbr, nbr_t, lists, rows = rulebook(dev, cin, cout, geo)
    w = sc.conv_weight(27, cin, cout, cin + 2 * cout)
    conv_backward_case(dev, f"conv{'' if geo[0] else ' s2'} {cin}->{cout} x{rows}", rb, nbr_t, lists, rows, rb.num_out, w)


def test_dense_conv_stack_backward_componentwise(dev):
    """dense_train.conv_stack's backward through autograd: one 12 x 12 map, 64 -> 64 channels, the dense-grid rulebook
    (border taps are ragged: 121 / 132 / 144 pairs) with WGRAD_FULL_TAPS"""
    from isfusion_amd import dense_train
    from isfusion_amd.dense_conv import grid_rulebook
    H = W = 12
    c = 64
    conv = torch.nn.Conv2d(c, c, 3, padding=1, bias=False).to(dev)
    w = sc.conv_weight(9, c, c, 5)                                                   # [(ky, kx), cin, cout]
    with torch.no_grad():
        conv.weight.copy_(T(w.reshape(3, 3, c, c), dev).permute(3, 2, 0, 1))
    rb = grid_rulebook(dev, 1, H, W, 1)
    nbr = np.maximum(rb.nbr.view(9, rb.stride)[:, :rb.num_out].cpu().numpy().astype(np.int64), -1)
    assert (nbr >= 0).sum(1).tolist() == (sc.dense_nbr(H, W) >= 0).sum(1).tolist() == [121, 132, 121, 132, 144, 132, 121, 132, 121]
    nbr_t, lists = sm.transpose_nbr(nbr, H * W), sm.pairs_from_nbr(nbr)
    assert dense_train.usable(conv)

    def run(x, g, half, want_dx, want_dw):
        xm = T(x, dev).view(1, H, W, c).permute(0, 3, 1, 2).requires_grad_()
        conv.weight.grad = None
        with torch.autocast("cuda", enabled=half):
            y = dense_train.conv_stack(conv, xm)
        y.backward(T(g, dev).view(1, H, W, c).permute(0, 3, 1, 2))
        dx = xm.grad.permute(0, 2, 3, 1).reshape(H * W, c).cpu().numpy()
        return dx, conv.weight.grad.permute(2, 3, 1, 0).reshape(9, c, c).cpu().numpy()

    conv_backward_case(dev, "dense conv_stack 64->64 12x12", rb, nbr_t, lists, H * W, H * W, w, run=run)


@pytest.mark.parametrize("M,R,O", sc.LINEAR_SHAPES)
def test_linear_function_dx_componentwise(dev, M, R, O):
    """fusion_train.LinearFunction's dX = G W (isf_grad_rescale, the forward GEMM on the transposed packed weight, fp32
    rows times 1 / s), every gradient class.  (M, R, O) is the shape of that GEMM, as in the forward tier's list: gradient
    rows [M, R], weight [R, O] (a Linear with O inputs and R outputs), dX [M, O].  O = 256 runs through autograd.  A Linear
    with 384 inputs has no forward on isf_linear_forward (in_features <= 256), so LinearFunction.apply cannot start there;
    its dX GEMM (1000 x 128 -> 384) is built, and LinearFunction.backward is called on a stand-in for the context the
    forward would have left."""
    import types
    from isfusion_amd import fusion_train
    w = sc.linear_weight(O, R, M + R + O)
    wd = T(w, dev)

    def run(g):
        if O <= 256:
            x = torch.zeros((M, O), device=dev, requires_grad=True)
            fusion_train.LinearFunction.apply(x, wd, None).backward(T(g, dev))
            return x.grad.cpu().numpy()
        ctx = types.SimpleNamespace(saved_tensors=(torch.zeros((M, O), device=dev), wd), needs_input_grad=(True, False, False),
                                    has_bias=False, in_dtype=torch.float32, _fwd_used_autocast=False, _dtype=torch.float16)
        return fusion_train.LinearFunction.backward(ctx, T(g, dev))[0].cpu().numpy()

    for cls in sm.GRAD_CLASSES:
        g = sm.make_grad(cls, (M, R), 43)
        y, bound = sm.linear_dgrad_model(g, w)
        assert np.isfinite(y).all() and np.abs(y).max() > 0
        got = run(g)
        check_bound(f"bwd LinearFunction dX {M}x{R}->{O}", cls, got, y, bound)
        if cls in ("Guni", "Grow"):
            equivariant(f"LinearFunction {M}x{R}->{O}", cls, (got, None), lambda f: (run(sc.factor(g, f)), None))


def rows_wgrad_cases():
    """(R, N, K, B, (H, W)): R = 130, the smallest R that isf_rows_weight_grad_chunks cuts into more than one chunk (its last
    chunk is then ragged: asserted), and R = 1000 on a wide dW (16 chunks of two steps, the last one 40 rows); NCHW maps
    with odd hw"""
    lib = _lib.load()
    N, K = sc.ROWS_WGRAD_SHAPES[0]
    rmin = next(r for r in range(1, 4096) if lib.isf_rows_weight_grad_chunks(r, N, K) > 1)
    assert rmin % 32 != 0 and rmin % 3 == 0
    N2, K2 = sc.ROWS_WGRAD_SHAPES[1]
    ch = lib.isf_rows_weight_grad_chunks(1000, N2, K2)
    assert ch > 2 and 1000 % ch != 0
    return [(130, N, K, 2, (5, 13)), (rmin, N, K, 3, (1, rmin // 3)), (1000, N2, K2, 8, (5, 25))]


def test_rows_weight_grad_componentwise(dev):
    """generalized_lss.rows_weight_grad as LateralFunction.backward calls it (the gradient through _lib.grad_rescale, its
    inverse scale as a device scalar), token-row and NCHW layouts of x: dW = G^T X / s, both operands split in the kernel"""
    from isfusion_amd import generalized_lss as lss
    for R, N, K, B, (H, W) in rows_wgrad_cases():
        assert B * H * W == R and (H * W) % 2 == 1

        def run(x, g):
            gs, scale = _lib.grad_rescale(T(g, dev))
            xm = np.ascontiguousarray(x.reshape(B, H * W, K).transpose(0, 2, 1)).reshape(B, K, H, W)
            return (lss.rows_weight_grad(gs, T(x, dev), scale[1:]).cpu().numpy(),
                    lss.rows_weight_grad(gs, T(xm, dev), scale[1:]).cpu().numpy())

        for gcls, xcls in sc.PAIRS:
            g = sm.make_grad(gcls, (R, N), 47)
            x = sm.make_class(xcls, (R, K), 53)
            m, bound = sm.rows_wgrad_model(g, x)
            assert np.isfinite(m).all() and np.abs(m).max() > 0
            got = run(x, g)
            for layout, a in zip(("rows", "NCHW"), got):
                check_bound(f"bwd rows_weight_grad R={R} {N}x{K} [{layout}]", f"{gcls} x {xcls}", a, m, bound)
            if gcls in ("Guni", "Grow"):
                equivariant(f"rows_weight_grad R={R} {N}x{K}", f"{gcls} x {xcls}", got, lambda f: run(x, sc.factor(g, f)))


# ------------------------------------------------------------------------------------------------ (e) non-finite
@pytest.mark.parametrize("cin,cout,geo", [(ci, co, sc.SUBM) for ci, co in sc.CONV_SHAPES] +
                         [(64, 64, sc.STRIDED), (128, 256, sc.STRIDED)],
                         ids=lambda v: ("subm" if v[0] else "stride2") if isinstance(v, tuple) else str(v))
def test_non_finite_gradients_are_loud_and_confined(dev, cin, cout, geo):
    """an infinity in gradient row 0, a NaN and a finite 3.2e38 (it overflows f16 once split) in two other rows, class-C
    activations: exactly the dX rows that read one of the three rows and the dW COLUMNS (tap, :, channel of the planted
    element) of the taps that pair one are non-finite; every other element meets its finite bound.  Row 0 is the row
    wgrad16_kernel loads for the positions past a pair list's end (the list's -1 padding clamped to 0): a tap that does
    not pair row 0 must not see it."""
    rb, nbr, nbr_t, lists, rows = rulebook(dev, cin, cout, geo)
    w = sc.conv_weight(27, cin, cout, cin + 2 * cout)
    g, planted = sc.poisoned_grad((rb.num_out, cout), cin + cout)
    x = sm.make_class("C", (rows, cin), 31)
    family = f"conv{'' if geo[0] else ' s2'} {cin}->{cout}"
    for half in (False, True):
        terms, scale = ((0, 0, 1), HALF_BOUND) if half else ((1, 1, 1), 1.0)
        tag = " [f16]" if half else ""
        dx, dw = run_backward(dev, rb, x, g, w, half=half)
        y, bound = sm.dgrad_model(g, w, nbr_t, rows, terms=terms)
        m, S, n = sm.wgrad_model(x, g, *lists, terms=terms)
        bad_x, bad_w = np.isnan(y), np.isnan(m)
        assert np.array_equal(bad_x, np.broadcast_to(np.isin(nbr_t, planted).any(0)[:, None], y.shape)) and bad_x.any()
        taps = np.array([np.isin(lists[1][k, :lists[2][k]], planted).any() for k in range(27)])
        assert np.array_equal(bad_w.any((1, 2)), taps) and 0 < taps.sum() < 27 and bad_w.sum() <= 3 * taps.sum() * cin
        for name, got, bad in (("dX", dx, bad_x), ("dW", dw, bad_w)):
            extra, missing = ~np.isfinite(got) & ~bad, np.isfinite(got) & bad
            print(f"split-domain bwd {family} {name}{tag} non-finite: {int(bad.sum())} elements in the model, "
                  f"{int(extra.sum())} more and {int(missing.sum())} fewer in the result"
                  + (f" (taps {sorted(set(np.nonzero(extra)[0].tolist()))})" if name == "dW" and extra.any() else ""))
            assert not extra.any() and not missing.any(), (family, name, tag)
        z = lambda a, bad: np.where(bad, 0, a)
        sb = sm.split_bound(z(y, bad_x))
        check_bound(f"bwd {family} dX{tag}", "non-finite", z(dx, bad_x), z(y, bad_x),
                    np.where(bad_x, 0, sb + (z(bound, bad_x) - sb) * scale), skip=bad_x)
        check_bound(f"bwd {family} dW{tag}", "non-finite", z(dw, bad_w), z(m, bad_w),
                    z(sm.wgrad_bound(S, n), bad_w) * scale, skip=bad_w)
