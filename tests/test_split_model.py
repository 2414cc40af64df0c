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
