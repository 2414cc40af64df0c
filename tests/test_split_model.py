"""The float64 model of the f16x3 split arithmetic (tests/split_model.py) checked on the CPU: the properties of the
format the GPU tier relies on, the tolerance of that tier shown to be met by an honest fp32 evaluation and MISSED by the
failures it is meant to catch (flushed f16 subnormals, a dropped lo*hi term), and the accuracy-vs-magnitude table the
documents quote (run with -s to see it)."""
import numpy as np
import pytest

import split_model as sm


@pytest.fixture(scope="module")
def values():
    """>= 1e6 fp32 values: log-uniform magnitudes over 2^-30 .. 65504, both signs, plus the edge values (class F)"""
    rng = np.random.default_rng(2024)
    n = 1_200_000
    mag = np.exp2(rng.uniform(-30.0, np.log2(sm.F16_MAX), n))
    x = (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    x = np.clip(x, -sm.F16_MAX, sm.F16_MAX)
    return np.concatenate([x, sm.EDGE_VALUES, sm.make_class("F", (64, 64), 3).ravel()])


def test_hi_plus_lo_is_exact_in_fp32(values):
    hi, lo = sm.split(values)
    assert np.array_equal(sm.join(hi, lo).astype(np.float64), hi.astype(np.float64) + lo.astype(np.float64))


def test_resplit_keeps_the_value_not_the_halves(values):
    """join(split(.)) is idempotent as a VALUE; the halves need not be (hi + lo can round to another hi when re-split),
    which is why the GPU tier compares joined values wherever a kernel re-splits.  The share of values whose halves change
    is printed: about 1 % on this log-uniform sample."""
    once = sm.join(*sm.split(values))
    h2, l2 = sm.split(once)
    assert np.array_equal(sm.join(h2, l2), once)
    h1, _ = sm.split(values)
    print(f"\nre-split changes the halves of {np.mean(h1.view(np.uint16) != h2.view(np.uint16)):.1%} of the values")


def test_roundtrip_error_bound(values):
    err = np.abs(sm.join(*sm.split(values)).astype(np.float64) - values.astype(np.float64))
    ratio = err / sm.split_bound(values)
    print(f"\nworst |join(split(x)) - x| / max(2^-22 |x|, 2^-25) = {ratio.max():.6f}")
    assert ratio.max() <= 1.0


def test_weight_scale_rule():
    rng = np.random.default_rng(5)
    for s in (1e-6, 3e-3, 0.0625, 0.99, 1.0, 4096.0, 8191.9, 8192.0, 1e7):
        w = (rng.uniform(-1, 1, 100) * s).astype(np.float32)
        top = float(np.abs(w).max()) * 2.0 ** sm.weight_scale(w)
        assert 2.0 ** 12 <= top < 2.0 ** 13, (s, top)
    assert sm.weight_scale(np.zeros(4, np.float32)) == 0


def _case(cls, seed, M=48, K=576, N=24):
    rng = np.random.default_rng(seed)
    a = sm.make_class(cls, (M, K), seed)
    w = rng.normal(0, (1.0 / K) ** 0.5, (N, K)).astype(np.float32)
    return a, w


@pytest.mark.parametrize("cls", sm.CLASSES)
def test_sequential_fp32_evaluation_stays_inside_the_bound(cls):
    a, w = _case(cls, 11)
    y, S, n = sm.gemm_model(a, w)
    got = sm.gemm_fp32_sequential(a, w).astype(np.float64)
    bound = sm.accumulation_bound(S, n)
    ok = bound > 0
    assert np.all(np.abs(got - y)[~ok] == 0)
    ratio = (np.abs(got - y)[ok] / bound[ok]).max()
    print(f"\nclass {cls}: fp32 sequential sum vs model, worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0


def _flush_ratio(scale_exp, K):
    rng = np.random.default_rng(17)
    M, N = 256, 64
    a = (rng.standard_normal((M, K)) * 2.0 ** scale_exp).astype(np.float32)
    w = rng.normal(0, (1.0 / K) ** 0.5, (N, K)).astype(np.float32)
    y, S, n = sm.gemm_model(a, w)
    bound = sm.accumulation_bound(S, n)
    honest = sm.gemm_fp32_sequential(a, w).astype(np.float64)
    assert (np.abs(honest - y) / bound).max() <= 1.0
    bad = sm.gemm_fp32_sequential(a, w, flush=True).astype(np.float64)
    return (np.abs(bad - y) / bound).max()


@pytest.mark.parametrize("scale_exp,K", [(-9, 64), (-10, 64), (-13, 64), (-17, 64), (-9, 128), (-10, 128), (-13, 128),
                                         (-17, 128), (-10, 576), (-13, 576), (-17, 576)])
def test_flushed_subnormals_leave_the_bound(scale_exp, K):
    """The failure the GPU tier exists to catch: a conversion that flushes f16 subnormal halves, at classes A (s = 2^-17)
    and B (s = 2^-9) and two scales between.  The honest evaluation is inside the bound, the flushed one outside by more
    than x20 -- at the term counts where the componentwise bound is the detector: the Linears (K <= 256), the Swin
    GEMMs' narrow layers and conv rows with few present taps.  The bound grows as n^2 (n terms, S a sum of n) and the
    flush error as sqrt(n), so the margin shrinks as n^-1.5: class B measures x352 / x102 at n = 64 / 128; at 576
    terms x21 at s = 2^-10, x458 at 2^-13, x2450 for class A.  Class B itself at 576 terms and conv-sized n is the
    subject of the next test."""
    ratio = _flush_ratio(scale_exp, K)
    print(f"\ns = 2^{scale_exp}, n = {K}: flushed conversion, worst error / bound = {ratio:.1f}")
    assert ratio > 20.0


def test_at_conv_sized_term_counts_the_exact_probe_is_the_detector_of_a_class_b_flush():
    """Class B (s = 2^-9) at 576 terms: a flushed conversion is only x9.3 outside the componentwise bound, and by the
    n^-1.5 law it is INSIDE it from n ~ 2500 on (a 3x3x3 conv on 128 or 256 channels has up to 3456 / 6912 terms).  So for
    the convs the bound is not what catches a class-B flush: the selection-matrix probes of the GPU tier are -- they
    compare with ==, whatever n.  Asserted here: (i) the measured margins, so the claim stays honest; (ii) that the probe
    fires: a flushed split changes join(split(x)) for most class-B and class-A values (every value whose lo -- or hi -- half
    is a non-zero subnormal), i.e. a kernel that flushes returns different values for them under a permutation weight."""
    r576 = _flush_ratio(-9, 576)
    print(f"\nclass B, n = 576: flushed conversion, worst error / bound = {r576:.1f}")
    assert 1.0 < r576 < 20.0
    rng = np.random.default_rng(17)
    a = (rng.standard_normal((64, 3456)) * 2.0 ** -9).astype(np.float32)
    w = rng.normal(0, (1.0 / 3456) ** 0.5, (16, 3456)).astype(np.float32)
    y, S, n = sm.gemm_model(a, w)
    yf, _, _ = sm.gemm_model(a, w, flush=True)
    r3456 = (np.abs(yf - y) / sm.accumulation_bound(S, n)).max()
    print(f"class B, n = 3456: flushed conversion, worst error / bound = {r3456:.2f} (inside: the bound cannot see it)")
    assert r3456 < 1.0
    for cls, share in (("B", 0.5), ("A", 0.5)):
        x = sm.make_class(cls, (256, 256), 1)
        changed = sm.join(*sm.split(x, flush=True)) != sm.join(*sm.split(x))
        print(f"class {cls}: the exact probe sees a flush on {changed.mean():.1%} of the values")
        assert changed.mean() > share
        assert changed.reshape(-1, 8).any(1).all()      # every 8-channel unit a lane converts holds such a value


def test_flushed_subnormals_change_class_a_and_b_bits():
    for cls in ("A", "B"):
        x = sm.make_class(cls, (64, 64), 1)
        h, l = sm.split(x)
        hf, lf = sm.split(x, flush=True)
        assert not np.array_equal(sm.join(h, l), sm.join(hf, lf)), cls


def test_dropped_lo_hi_term_leaves_the_bound_for_class_c():
    """the other sanity check of the GPU tier: a model (or kernel) without the a_lo * w_hi product is outside the bound
    at O(1) operands -- at the term counts of the Linears, the Swin GEMMs and conv rows with few taps (n <= 256: measured
    x13.8 at n = 64, x5.3 at 128).  The margin shrinks as n^-1.5 here too: at 576 terms the dropped term is INSIDE the
    bound (x0.5), which is why tier (b) of the GPU tests compares exactly instead."""
    for K in (64, 128):
        a, w = _case("C", 23, M=256, K=K, N=64)
        y, S, n = sm.gemm_model(a, w)
        y2, _, _ = sm.gemm_model(a, w, terms=(0, 1, 1))
        ratio = (np.abs(y2 - y) / sm.accumulation_bound(S, n)).max()
        print(f"\nclass C, n = {K}, without a_lo*w_hi: worst error / bound = {ratio:.1f}")
        assert ratio > 3.0
        got = sm.gemm_fp32_sequential(a, w).astype(np.float64)
        assert (np.abs(got - y2) / sm.accumulation_bound(S, n)).max() > 3.0


def test_conv_model_equals_gemm_model_on_a_one_tap_rulebook():
    a, w = _case("E_row", 31, M=40, K=64, N=32)
    nbr = np.arange(40, dtype=np.int32)[None, :].copy()
    nbr[0, 7] = -1
    y, S, n = sm.conv_model(a, w.T[None], nbr, 40)
    yg, Sg, _ = sm.gemm_model(a, w)
    yg[7], Sg[7] = 0, 0
    assert np.array_equal(y, yg) and np.array_equal(S, Sg) and n[7, 0] == 0 and n[0, 0] == 64


def test_overflow_poisons_whole_rows_and_nothing_else():
    x, rows = sm.make_overflow((64, 96), 9)
    w = np.random.default_rng(1).normal(0, 0.1, (32, 96)).astype(np.float32)
    w[:, ::2] = 0          # inf * 0 = NaN as well
    y, S, _ = sm.gemm_model(x, w)
    bad = np.zeros(64, bool)
    bad[rows] = True
    assert np.isnan(y[bad]).all() and np.isfinite(y[~bad]).all() and np.isfinite(S[~bad]).all()
    # the elements themselves: >= 65520, the infinities and NaN all join to NaN; 65519.9 stays finite
    assert np.isnan(sm.join(*sm.split(sm.OVERFLOW_VALUES))).all()
    assert np.isfinite(sm.join(*sm.split(np.float32(65519.9))))


def test_accuracy_table():
    """(model - exact) / max|exact| of a 576-term dot product against the activation magnitude: relative 2^-22 only while
    |a| >= 2^-3; absolute 2^-25 per element below; NaN from 65520 up"""
    table = sm.accuracy_table()
    print("\n  max|a|      rel. error of the f16x3 model (576 terms, N(0,1)*s activations, N(0,1/576) weights)")
    for amax, err in table:
        print(f"  {amax:10.3g}  {err:.2g}")
    errs = [e for _, e in table]
    assert errs[0] < 3e-7 and errs[1] < 6e-7           # both halves normal: fp32 class
    assert all(b > a for a, b in zip(errs[1:7], errs[2:8]))   # degrades monotonically below 2^-3
    assert errs[7] > 1e-3 and np.isnan(errs[8])


# ------------------------------------------------------------------------------------------------ the fused blocks
# The GPU tier judges attention, the window block and the DynamicVFE by bounds composed of several stages
# (tests/split_blocks.py).  Here each of those bounds is shown to be LEFT by the same composition with a flushing
# conversion on the activation side -- so a kernel that flushed there could not pass -- and where a bound cannot see a
# flush, that is measured and said.
def _worst(model, flushed_model, bound):
    return float((np.abs(flushed_model - model) / bound).max())


def test_attention_bound_sees_a_flushed_v_and_flushed_probabilities():
    """V at class B under O(1) queries and keys: a flushed V is outside the bound (measured x68 at Lk = 200, x17 at 700).  Flushed PROBABILITIES
    are inside it there (x0.8 / x0.2: the outputs are carried by the large probabilities), which is why the GPU test has the
    attention_small_probabilities case: there they are outside (x340 at Lk = 200, x140 at 700)."""
    import split_blocks as sb
    B, Lq, E = 2, 64, 128
    for Lk in (200, 700):
        rng = np.random.default_rng(Lk)
        q = rng.standard_normal((B * Lq, E)).astype(np.float32)
        k = rng.standard_normal((B * Lk, E)).astype(np.float32)
        v = sm.make_class("B", (B * Lk, E), 67)
        y, bound = sb.attention_model(q, k, v, B, Lq, Lk)
        rv = _worst(y, sb.attention_model(q, k, v, B, Lq, Lk, flush=("v",))[0], bound)
        rp = _worst(y, sb.attention_model(q, k, v, B, Lq, Lk, flush=("p",))[0], bound)
        q, k, v = sb.attention_small_probabilities(B, Lq, Lk)
        y, bound = sb.attention_model(q, k, v, B, Lq, Lk)
        rs = _worst(y, sb.attention_model(q, k, v, B, Lq, Lk, flush=("p",))[0], bound)
        print(f"\nattention Lk = {Lk}: flushed V (class B) x{rv:.1f}; flushed probabilities x{rp:.2f} under random operands, "
              f"x{rs:.1f} on the small-probability operands")
        assert rv > 10.0 and rs > 20.0 and rp < 1.0


def test_window_block_class_tolerance_sees_a_flush():
    """The window block's class check (difference to the class-C layer against the model's difference).  A flush of the
    attention output the out-projection re-splits leaves the tolerance by x10 with V at class B and by x24 at 2^-13; a
    flush of V by x13 at 2^-13 but only x2.1 at class B (36 keys and 128 out-projection terms average the random flush
    errors, the tolerance adds worst cases), so for V the 2^-13 case is the detector.  At class D nothing is subnormal: a
    flush changes nothing there, that case guards the large side (1e-3 of an output)."""
    import split_blocks as sb
    x = sb.window_block_input()
    for name, vs, need_v, need_att in (("B", 2.0 ** -9, 1.0, 5.0), ("2^-13", 2.0 ** -13, 5.0, 5.0)):
        pair = (vs, 1.0)
        base = sb.window_block_model(sb.window_block_layer(1.0, 0, pair), x, 0)
        layer = sb.window_block_layer(vs, 0, pair)
        other = sb.window_block_model(layer, x, 0, vref=base["vj"] * vs)
        tol = sb.window_block_class_tolerance(base, other)
        assert (np.abs(other["out"] - base["out"]) <= tol).all()             # the honest composition is inside
        rv = _worst(other["out"], sb.window_block_model(layer, x, 0, flush=("v",))["out"], tol)
        ra = _worst(other["out"], sb.window_block_model(layer, x, 0, flush=("att",))["out"], tol)
        full = _worst(other["out"], sb.window_block_model(layer, x, 0, flush=("v", "att"))["out"], other["full"])
        print(f"\nwindow block, V at {name}: flushed V x{rv:.1f}, flushed attention output x{ra:.1f} of the class tolerance "
              f"(median {np.median(tol):.2g}); both x{full:.2f} of the closeness bound")
        assert rv > need_v and ra > need_att
        assert full < 1.0 or vs < 2.0 ** -9                                 # the closeness bound cannot see a class-B flush


def test_vfe_offsets_only_bound_sees_a_flush():
    """The DynamicVFE variant whose layers see class A / B operands alone: a flush in layer 1's conversion leaves the bound
    by x9, one in layer 2's by x26.  With the seeded weights (|xyz|, intensity in the sums) both stay inside: printed."""
    import split_blocks as sb
    pts, coors = sb.vfe_cloud(3, 600, True, 255.0)
    f, inv, vc = sb.vfe_features(pts, coors)
    for offsets_only in (True, False):
        lb = sb.vfe_branch(offsets_only)
        want, bound = sb.vfe_model(lb, f, inv, len(vc))
        r1 = _worst(want, sb.vfe_model(lb, f, inv, len(vc), flush=(1,))[0], bound)
        r2 = _worst(want, sb.vfe_model(lb, f, inv, len(vc), flush=(2,))[0], bound)
        print(f"\nDynamicVFE, {'offset features only' if offsets_only else 'seeded weights'}: flushed layer-1 operands "
              f"x{r1:.2f}, flushed layer-2 operands x{r2:.2f} of the bound")
        assert (r1 > 5.0 and r2 > 5.0) if offsets_only else (r1 < 1.0 and r2 < 1.0)


# ------------------------------------------------------------------------------------------------ the backward
# tests/test_gpu_split_backward.py judges dX and dW per element by  3 n 2^-24 S / s  (+ the split store for dX).  Here, on
# that file's own inputs (tests/split_backward_cases.py; the rulebooks restated in numpy), each of those bounds is shown
# to be MET by an fp32 evaluation of the same halves (BLAS sgemm per product and tap, summed in fp32: one of the orders a
# kernel may use) and LEFT by each of seven defects:
#   1 the gradient halves flush f16 subnormals      2 the x halves do (dW only: dX reads no activations)
#   3-5 one of the three products is missing        6 the scale comes from the wrong element
#   7 the inverse scale is not applied to one chunk
# A ratio is max |defect - model| / bound over the elements the model keeps finite; a defect that makes such an element
# non-finite counts as infinitely far out.  Where a class cannot see a defect the ratio is printed and the reason given.
def _f32(h):
    return h.astype(np.float32)


def _three32(ah, al, wh, wl):
    return _f32(al) @ _f32(wh) + _f32(ah) @ _f32(wl) + _f32(ah) @ _f32(wh)


def _wgrad32(x, g, pin, pout, counts):
    s = sm.grad_scale(g)
    (xh, xl), (gh, gl) = sm.split(x), sm.split(sm.scaled(g, s))
    out = np.zeros((len(counts), x.shape[1], g.shape[1]), np.float32)
    for k in range(len(counts)):
        i, o = pin[k, :counts[k]], pout[k, :counts[k]]
        for c in range(0, counts[k], 256):               # pair chunks of 256, partial blocks added in order
            out[k] += _three32(xh[i[c:c + 256]].T, xl[i[c:c + 256]].T, gh[o[c:c + 256]], gl[o[c:c + 256]])
    return out * np.float32(1.0 / s)


def _dgrad32(g, w, nbr_t, num_in):
    s = sm.grad_scale(g)
    gh, gl = sm.split(sm.scaled(g, s))
    wh, wl, sw = sm.split_weight(np.ascontiguousarray(w.transpose(0, 2, 1)))
    y = np.zeros((num_in, w.shape[1]), np.float32)
    for k in range(w.shape[0]):
        m = nbr_t[k] >= 0
        if m.any():
            y[m] += _three32(gh[nbr_t[k, m]], gl[nbr_t[k, m]], wh[k], wl[k])
    return sm.store_split(np.ldexp(y, -sw)) * np.float32(1.0 / s)


def _ratio(defect, model, bound):
    ok = np.isfinite(model)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(defect - model)[ok]
        r = np.where(err == 0, 0.0, err / bound[ok])
    return float("inf") if not np.isfinite(r).all() else float(r.max())


def _conv_case(cin, cout, geo):
    import split_backward_cases as sc
    rows = sc.conv_rows(cin, cout)
    nbr, num_out = sc.cpu_nbr(sc.geometry(cin + cout, rows), sc.GRID, geo)
    sc.check_rulebook(nbr, 4, chunks3=geo[0])
    return rows, num_out, sm.transpose_nbr(nbr, rows), sm.pairs_from_nbr(nbr), sc.conv_weight(27, cin, cout, cin + 2 * cout)


BWD_CONV_CASES = [(32, 32, "subm"), (64, 64, "subm"), (64, 64, "stride2")]


@pytest.mark.parametrize("cin,cout,geo", BWD_CONV_CASES)
def test_backward_conv_bounds_hold_for_an_fp32_evaluation_and_see_the_seven_defects(cin, cout, geo):
    """dX and dW of the sparse conv on the GPU tier's rulebooks, gradient and activation classes.  Every defect must leave
    its bound for at least one class (asserted); measured at 64 -> 64 (printed for each case):
      * flushed gradient halves: dX x1600 (Grow), x2000 (Gspike), x2.6 (Gelem); dW x1e4 (Gspike x D), x6 (Gelem), x2 (Grow x
        E_row).  Guni and Gedge cannot see them: Guni's rows are O(max), its lo halves normal f16 numbers, and Gedge's few
        subnormal values drown in sums carried by its values of order one (x0.8 / x0.02);
      * flushed x halves (dW): x1e4 with x at class A, x900 at B, x3.5 at C; D and the E classes are inside (nothing
        subnormal at D; at E the large rows carry the sums);
      * a missing lo product: dX x13 .. x42, dW x3 .. x15 -- except where the operand has no lo half: Gspike for g_lo (600 and
        values of one or two bits), class A for x_lo (x0); a missing hi*hi product x1e4 everywhere;
      * a scale taken from the finite 3.2e38 of the non-finite test's gradient (s = 2^-118) zeroes every finite row (x6e4,
        x1e4); one taken from the tensor's smallest element overflows the large rows (non-finite: counted as infinite);
      * an inverse scale that skips one chunk cannot be seen at s = 1 (the classes as built: x0, asserted) and is x6e16 /
        x6e4 outside on the scale-equivariance inputs (the gradient times 2^-40 / 2^30)."""
    import split_backward_cases as sc
    rows, num_out, nbr_t, lists, w = _conv_case(cin, cout, sc.SUBM if geo == "subm" else sc.STRIDED)
    pin, pout, counts = lists
    big = int(np.argmax(counts))
    seen = {}
    note = lambda d, cls, r: seen.setdefault(d, {}).__setitem__(cls, r)
    for gcls, xcls in sc.PAIRS:
        g, x = sm.make_grad(gcls, (num_out, cout), 13), sm.make_class(xcls, (rows, cin), 31)
        y, bx = sm.dgrad_model(g, w, nbr_t, rows)
        m, S, n = sm.wgrad_model(x, g, *lists)
        bw = sm.wgrad_bound(S, n)
        assert _ratio(_dgrad32(g, w, nbr_t, rows).astype(np.float64), y, bx) <= 1.0, (gcls, "dX fp32")
        assert _ratio(_wgrad32(x, g, *lists).astype(np.float64), m, bw) <= 1.0, (gcls, xcls, "dW fp32")
        cls = f"{gcls} x {xcls}"
        note("dX flushed g", cls, _ratio(sm.dgrad_model(g, w, nbr_t, rows, flush=True)[0], y, bx))
        note("dW flushed g", cls, _ratio(sm.wgrad_model(x, g, *lists, flush="g")[0], m, bw))
        note("dW flushed x", cls, _ratio(sm.wgrad_model(x, g, *lists, flush="x")[0], m, bw))
        for i, name in enumerate(("lo*hi", "hi*lo", "hi*hi")):
            terms = tuple(int(j != i) for j in range(3))
            note(f"dX without g_{name.replace('*', '*w_')}", cls, _ratio(sm.dgrad_model(g, w, nbr_t, rows, terms=terms)[0], y, bx))
            note(f"dW without x_{name.replace('*', '*g_')}", cls, _ratio(sm.wgrad_model(x, g, *lists, terms=terms)[0], m, bw))
        tiny = float(np.abs(g[g != 0]).min())
        s_bad = sm.grad_scale(np.array([tiny], np.float32))
        note("dX scale from the smallest element", cls, _ratio(sm.dgrad_model(g, w, nbr_t, rows, s=s_bad)[0], y, bx))
        note("dW scale from the smallest element", cls, _ratio(sm.wgrad_model(x, g, *lists, s=s_bad)[0], m, bw))
        for f in (1.0,) + (sc.FACTORS if gcls in ("Guni", "Grow") else ()):
            gf = sc.factor(g, f)
            s = sm.grad_scale(gf)
            yf, bxf = sm.dgrad_model(gf, w, nbr_t, rows)
            mf, Sf, nf = sm.wgrad_model(x, gf, *lists)
            skipped = yf.copy()
            skipped[256:512] *= s                                    # rows 256 .. 511 never multiplied by 1 / s
            chunk = sm.wgrad_model(x, gf, pin[:, :256], pout[:, :256], np.minimum(counts, 256))[0][big]
            part = mf.copy()
            part[big] += chunk * (s - 1.0)                           # the first chunk of the longest tap likewise
            tag = cls if f == 1.0 else f"{cls} x 2^{int(np.log2(f))}"
            note("dX inverse scale skips a chunk", tag, _ratio(skipped, yf, bxf))
            note("dW inverse scale skips a chunk", tag, _ratio(part, mf, sm.wgrad_bound(Sf, nf)))
    g, planted = sc.poisoned_grad((num_out, cout), cin + cout)
    x = sm.make_class("C", (rows, cin), 31)
    y, bx = sm.dgrad_model(g, w, nbr_t, rows)
    m, S, n = sm.wgrad_model(x, g, *lists)
    s_bad = 2.0 ** (10 - int(np.frexp(np.float32(3.2e38))[1]))
    note("dX scale from the 3.2e38 entry", "non-finite", _ratio(sm.dgrad_model(g, w, nbr_t, rows, s=s_bad)[0], y, bx))
    note("dW scale from the 3.2e38 entry", "non-finite", _ratio(sm.wgrad_model(x, g, *lists, s=s_bad)[0], m, sm.wgrad_bound(S, n)))
    print()
    for d, per in seen.items():
        print(f"conv {cin}->{cout} {geo}, {d}: " + ", ".join(f"{c} x{r:.3g}" for c, r in per.items()))
        assert max(per.values()) > 2.0, (d, per)
    inside = lambda d, c: seen[d][c] <= 1.0
    assert inside("dX flushed g", "Guni x C") and inside("dW flushed x", "Guni x C") and inside("dW flushed x", "Gspike x D")
    assert all(inside(f"{t} inverse scale skips a chunk", f"{c[0]} x {c[1]}") for t in ("dX", "dW") for c in sc.PAIRS)


def test_backward_gemm_bounds_hold_for_an_fp32_evaluation_and_see_the_seven_defects():
    """the dense-GEMM forms on the GPU tier's shapes: LinearFunction's dX (700 x 256 -> 256) and isf_rows_weight_grad
    (R = 130, 64 x 96), same defects (for dX a flush of the x halves does not exist: the weight is the other operand and
    is packed at 2^12, nothing of it is subnormal).  The dX bound is the one that counts subnormal halves as 2^-14
    (split_model.linear_dgrad_model): every defect still leaves it -- flushed gradient halves by x2900 (Grow) and x3400
    (Gspike), a missing product by x2 .. x20 (the two lo products) and x1e4 (hi*hi); Guni and Gelem cannot see a flush."""
    import split_backward_cases as sc
    M, N, K = sc.LINEAR_SHAPES[0]                                    # gradient [M, N], weight [N, K]
    w = sc.linear_weight(K, N, M + K + N)
    R, (N2, K2) = 130, sc.ROWS_WGRAD_SHAPES[0]
    seen = {}
    note = lambda d, cls, r: seen.setdefault(d, {}).__setitem__(cls, r)
    for gcls, xcls in sc.PAIRS:
        g = sm.make_grad(gcls, (M, N), 43)
        y, by = sm.linear_dgrad_model(g, w)
        gh, gl = sm.split(g)
        wh, wl, sw = sm.split_weight(w)
        assert sm.grad_scale(g) == 1.0 and _ratio(np.ldexp(_three32(gh, gl, wh, wl), -sw).astype(np.float64), y, by) <= 1.0
        g2, x2 = sm.make_grad(gcls, (R, N2), 47), sm.make_class(xcls, (R, K2), 53)
        m, bm = sm.rows_wgrad_model(g2, x2)
        g2h, g2l = sm.split(g2)
        x2h, x2l = sm.split(x2)
        fp32 = np.zeros(m.shape, np.float32)
        for c in range(0, R, 32):                                    # row chunks, partial blocks added in order
            fp32 += _three32(g2h[c:c + 32].T, g2l[c:c + 32].T, x2h[c:c + 32], x2l[c:c + 32])
        assert _ratio(fp32.astype(np.float64), m, bm) <= 1.0
        cls = f"{gcls} x {xcls}"
        note("linear dX flushed g", gcls, _ratio(sm.linear_dgrad_model(g, w, flush=True)[0], y, by))
        note("rows dW flushed g", cls, _ratio(sm.rows_wgrad_model(g2, x2, flush="g")[0], m, bm))
        note("rows dW flushed x", cls, _ratio(sm.rows_wgrad_model(g2, x2, flush="x")[0], m, bm))
        for i, name in enumerate(("lo*hi", "hi*lo", "hi*hi")):
            terms = tuple(int(j != i) for j in range(3))
            note(f"linear dX without g_{name.replace('*', '*w_')}", gcls, _ratio(sm.linear_dgrad_model(g, w, terms=terms)[0], y, by))
            note(f"rows dW without g_{name.replace('*', '*x_')}", cls, _ratio(sm.rows_wgrad_model(g2, x2, terms=terms)[0], m, bm))
        for gg, d, fn in ((g, "linear dX", lambda s: sm.linear_dgrad_model(g, w, s=s)[0]),
                          (g2, "rows dW", lambda s: sm.rows_wgrad_model(g2, x2, s=s)[0])):
            for what, el in (("smallest element", float(np.abs(gg[gg != 0]).min())), ("a 3.2e38 entry", 3.2e38)):
                ref, b = (y, by) if d == "linear dX" else (m, bm)
                note(f"{d} scale from {what}", cls, _ratio(fn(2.0 ** min(10 - int(np.frexp(np.float32(el))[1]), 126)), ref, b))
        for f in (1.0,) + (sc.FACTORS if gcls in ("Guni", "Grow") else ()):
            tag = cls if f == 1.0 else f"{cls} x 2^{int(np.log2(f))}"
            gf, g2f = sc.factor(g, f), sc.factor(g2, f)
            s = sm.grad_scale(gf)
            yf, bf = sm.linear_dgrad_model(gf, w)
            skipped = yf.copy()
            skipped[256:512] *= s
            note("linear dX inverse scale skips a chunk", tag, _ratio(skipped, yf, bf))
            mf, bmf = sm.rows_wgrad_model(g2f, x2)
            part = sm.rows_wgrad_model(g2f[:32], x2[:32], s=s)[0]
            note("rows dW inverse scale skips a chunk", tag, _ratio(mf + part * (s - 1.0), mf, bmf))
    print()
    for d, per in seen.items():
        print(f"{d}: " + ", ".join(f"{c} x{r:.3g}" for c, r in per.items()))
        assert max(per.values()) > 2.0, (d, per)


def test_grad_scale_rule():
    """s = 2^(10 - e): the largest entry lands in [2^9, 2^10); clamped to 2^126 for a denormal maximum; 1 for zeros; inf,
    NaN and finite entries above 3.0e38 do not set it"""
    rng = np.random.default_rng(9)
    for mag in (1e-30, 3e-9, 1e-6, 0.4999, 0.5, 1.0, 511.9, 512.0, 1023.9, 1024.0, 1e20, 2.9e38):
        g = (rng.uniform(-1, 1, 100) * mag).astype(np.float32)
        assert 2.0 ** 9 <= float(np.abs(g).max()) * sm.grad_scale(g) < 2.0 ** 10, mag
    assert sm.grad_scale(np.zeros(8, np.float32)) == 1.0
    assert sm.grad_scale(np.array([1e-40, -3e-41], np.float32)) == 2.0 ** 126
    assert sm.grad_scale(np.array([np.inf, -np.inf, np.nan, 3.2e38, 600.0], np.float32)) == 1.0
    assert sm.grad_scale(np.array([np.inf, np.nan], np.float32)) == 1.0
    for cls in sm.GRAD_CLASSES:
        assert sm.grad_scale(sm.make_grad(cls, (130, 64), 1)) == 1.0


def test_backward_accuracy_table():
    """relative error of a gradient row's dX and dW contribution against the row's magnitude relative to the tensor's
    maximum: fp32 class down to 2^-12, 2^-25 absolute per element below (lo subnormal), half the bits gone at 2^-24, the
    row lost from 2^-34 on (|g s| < 2^-25 rounds to zero)"""
    table = sm.backward_accuracy_table()
    print("\n  row / max   rel. error of dX    of dW   (f16x3 model against exact float64, 256-term Linear)")
    for k, ex, ew in table:
        print(f"  2^-{k:<8d}  {ex:.2g}          {ew:.2g}")
    err = {k: (ex, ew) for k, ex, ew in table}
    assert max(err[0]) < 3e-7 and max(err[12]) < 1e-6
    assert all(err[b][i] > err[a][i] for a, b in ((13, 16), (16, 20), (20, 24), (24, 28), (28, 32)) for i in (0, 1))
    assert min(err[24]) > 5e-4 and err[35] == (1.0, 1.0) and err[40] == (1.0, 1.0)
