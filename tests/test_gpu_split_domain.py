"""The split-precision ("f16x3") kernels across the whole f16 magnitude range (-m gpu).

Every matrix-core kernel of the forward path converts its fp32 operands to f16 hi/lo halves with conversion code of its
own.  The rest of the GPU tier feeds them O(1) operands and divides errors by the tensor's maximum, so a family that
flushed f16 subnormals, truncated, or dropped a lo term on some lanes would pass it.  Here each family is judged per
output element against tests/split_model.py (the same halves, the same three products, summed in float64), on operands of
every magnitude class:

    A  hi subnormal (s = 2^-17)       B  lo subnormal (s = 2^-9)      C  both normal (s = 1)      D  large (s = 2^12)
    E  mixed per row / per element (2^-20 .. 2^13)      F  edge values      G  overflow (>= 65520, inf, NaN) in class C

  (a) the conversion kernels, bit for bit;
  (b) selection-matrix probes: a weight of single 1.0 entries makes every product and sum exact, so the output must EQUAL
      join(split(x)) of the selected input -- each family's in-kernel conversion, its gathers and its absent-neighbour
      masking observed exactly (compared as values: a kernel that stores split rows re-splits, and the halves of a value
      are not unique);
  (c) random operands: |y - model| <= 3 n 2^-24 S + E_store per output element (split_model.accumulation_bound: the
      worst fp32 accumulation of the 3 n exact products in any order; E_store: max(2^-22 |y|, 2^-25) for split-stored
      outputs, 2^-23 |y| per fp32 epilogue operation) -- no tuned number.  The bounds of GELU, LayerNorm, attention, the
      window block and the DynamicVFE compose that form over several stages with constants derived, one by one, where each
      is defined (here and in tests/split_blocks.py); tests/test_split_model.py shows for each composed bound which flushed
      conversion leaves it, and says where one does not;
  (d) overflow (class G) is loud, confined to the outputs that read a poisoned row, and never finite-wrong.

Each check prints one line `split-domain <family> <class>: ...` with the worst error / bound ratio, or that the probe
was met exactly (run with -s)."""
import numpy as np
import pytest
import torch

import split_blocks as sb
import split_model as sm
from isfusion_amd import _lib

pytestmark = pytest.mark.gpu

FINITE = sm.CLASSES                     # A, B, C, D, E_row, E_elem, F
RANDOM = ("A", "B", "C", "D", "E_row", "E_elem")
U23 = sb.U23                            # one fp32 rounding, relative (2 u: also covers a fused or unfused multiply-add)


def T(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def geometry(seed, B, shape, n):
    rng = np.random.default_rng([seed, 5])
    cells = B * int(np.prod(shape))
    lin = np.sort(rng.choice(cells, n, replace=False))
    D, H, W = shape
    return np.stack([lin // (D * H * W), (lin // (H * W)) % D, (lin // W) % H, lin % W], 1).astype(np.int32)


def report(family, cls, ratio):
    print(f"split-domain {family} {cls}: worst error / bound = {ratio:.3g}")


def check_bound(family, cls, got, y, bound, skip=None):
    """per element |got - y| <= bound (== where the bound is 0); skip: mask of elements judged elsewhere"""
    got = (got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)).astype(np.float64)
    keep = np.ones(y.shape, bool) if skip is None else ~skip
    assert np.isfinite(got[keep]).all(), (family, cls, "non-finite output where the model is finite")
    err = np.abs(got - y)
    zero = keep & (bound == 0)
    assert (err[zero] == 0).all(), (family, cls, "output differs where the model allows no error")
    pos = keep & (bound > 0)
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    report(family, cls, ratio)
    assert ratio <= 1.0, (family, cls, ratio)
    return ratio


def check_equal(family, cls, got, want):
    """== as values (-0 equals +0)"""
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    bad = got != want
    assert not bad.any(), (family, cls, int(bad.sum()), got[bad][:4], want[bad][:4])


def report_exact(family, cls, what=""):
    print(f"split-domain {family} {cls}: equal to join(split(x)) of the selected input{what}")


# ------------------------------------------------------------------------------------------------ (a) conversions
def _is_nan16(bits):
    return (bits & 0x7FFF) > 0x7C00


@pytest.mark.parametrize("cls", FINITE + ("G",))
def test_conversion_kernels_bit_for_bit(dev, cls):
    """isf_f32_to_split == the model's hi / lo BITS (the conversion of a given fp32 value is deterministic), from_split ==
    join, to_half / from_half == numpy's float16 conversion.  NaNs are compared as NaNs: IEEE leaves their sign and
    payload open (inf - inf is -qNaN on x86 and +qNaN on the GPU)."""
    from isfusion_amd import spconv as sp
    x = sm.make_overflow((1024, 64), 3)[0] if cls == "G" else sm.make_class(cls, (1024, 64), 3)
    want = sm.to_split_bytes(x)
    got = sp.to_split(T(x, dev)).cpu().numpy().view(np.uint16).reshape(want.shape)
    nan = _is_nan16(want)
    assert np.array_equal(_is_nan16(got), nan) and np.array_equal(got[~nan], want[~nan]), cls
    assert cls == "G" or not nan.any()
    back = sp.from_split(T(want.view(np.uint8).ravel(), dev), x.shape).cpu().numpy()
    wj = sm.join(*sm.split(x))
    ok = ~np.isnan(wj)
    assert np.array_equal(np.isnan(back), ~ok) and np.array_equal(back[ok].view(np.uint32), wj[ok].view(np.uint32)), cls
    with np.errstate(over="ignore"):
        wh = x.astype(np.float16)
    gh = sp.to_half(T(x, dev)).cpu().numpy().view(np.uint16).reshape(x.shape)
    nanh = np.isnan(wh)
    assert np.array_equal(_is_nan16(gh), nanh) and np.array_equal(gh[~nanh], wh.view(np.uint16)[~nanh]), cls
    report("to_split / from_split / to_half (bits)", cls, 0.0)


def test_from_half_and_from_split_on_every_f16_pattern(dev):
    from isfusion_amd import spconv as sp
    bits = np.arange(65536, dtype=np.uint16)
    want = bits.view(np.float16).astype(np.float32)
    got = sp.from_half(T(bits.view(np.uint8), dev), (2048, 32)).cpu().numpy().ravel()
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok) and np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))
    rng = np.random.default_rng(1)
    hl = rng.integers(0, 65536, (4096, 2, 32), dtype=np.uint16)          # random halves, subnormal and non-finite included
    want = sm.join(hl[:, 0].view(np.float16), hl[:, 1].view(np.float16)).ravel()
    got = sp.from_split(T(hl.view(np.uint8).ravel(), dev), (4096, 32)).cpu().numpy().ravel()
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok) and np.array_equal(got[ok], want[ok])


# ------------------------------------------------------------------------------------------------ conv plumbing
F16X3_MODES = (("mode 0", 0), ("no sharing", _lib.CONV_MODE_NO_SHARING), ("uniform tiles", _lib.CONV_MODE_UNIFORM_TILES))


def conv_entries(cin, cout, n_out):
    """(name, callable(sp, x, p16, K, rb, scale, shift, residual, relu) -> fp32 rows) of every entry point built for the
    shape"""
    out = []
    for name, mode in F16X3_MODES:
        out.append((f"f16x3 {name}", lambda sp, x, p, K, rb, sc, sh, rs, relu, mode=mode:
                    sp.sparse_conv_forward_f16x3(x, p, K, cin, cout, rb, sc, sh, rs, relu, mode=mode)))
    if cin >= 128 and cout == 256:
        out.append(("f16x3 deep", lambda sp, x, p, K, rb, sc, sh, rs, relu:
                    sp.sparse_conv_forward_f16x3(x, p, K, cin, cout, rb, sc, sh, rs, relu, mode=_lib.CONV_MODE_DEEP)))
        out.append(("cu", lambda sp, x, p, K, rb, sc, sh, rs, relu:
                    sp.sparse_conv_forward_cu(x, p, K, cin, cout, rb, sc, sh, rs, relu)))
    if cin <= 64 and cout <= 64:
        out.append(("dma", lambda sp, x, p, K, rb, sc, sh, rs, relu:
                    sp.sparse_conv_forward_dma(x, p, K, cin, cout, rb, sc, sh, rs, relu)))
    for rows in (96, 512):
        out.append((f"staged {rows}", lambda sp, x, p, K, rb, sc, sh, rs, relu, rows=rows:
                    sp.sparse_conv_forward_staged(x, p, K, cin, cout, rb, sc, sh, rs, relu, stage_rows=rows)))
    return out


# (cin, cout, rows, grid): each channel shape the launcher dispatches differently; 2600 rows put the 128-column shapes on
# the 8-wave tile; 30000 rows put the 256-column shape above the small-launch bound, where the two-group kernel with the
# assembly multiply section and (CONV_MODE_DEEP) isf_spconv_deep.hip run
CONV_SHAPES = [(32, 32, 2600, [9, 40, 36]), (64, 64, 2600, [9, 40, 36]), (64, 128, 2600, [9, 40, 36]),
               (128, 128, 2600, [9, 40, 36]), (256, 256, 2600, [9, 40, 36]), (128, 256, 700, [9, 24, 20]),
               (256, 256, 30000, [12, 96, 96])]
SUBM = (True, [3, 3, 3], [1, 1, 1], [1, 1, 1])
STRIDED = (False, [3, 3, 3], [2, 2, 2], [1, 1, 1])


def build_rb(sp, dev, seed, rows, grid, geo=SUBM):
    subm, ks, st, pd = geo
    idx = geometry(seed, 2, grid, rows)
    rb = sp.build_rulebook(T(idx, dev), 2, grid, ks, st, pd, subm)
    K = int(np.prod(ks))
    nbr = rb.nbr.view(K, rb.stride)[:, :rb.num_out].cpu().numpy()
    return rb, nbr, K


def selection_weight(K, cin, cout, seed, taps):
    """w [K, cin, cout] of single 1.0 entries: output column c takes tap t(c), channel pi(c) -> (w, t, pi)"""
    rng = np.random.default_rng([seed, 9])
    pi = np.concatenate([rng.permutation(cin) for _ in range((cout + cin - 1) // cin)])[:cout]
    t = np.asarray(taps)[rng.integers(0, len(taps), cout)]
    w = np.zeros((K, cin, cout), np.float32)
    w[t, pi, np.arange(cout)] = 1.0
    return w, t, pi


def selected(xj, nbr, t, pi):
    """xj[nbr[t(c)][o]][pi(c)], 0 where the neighbour is absent"""
    src = nbr[t, :].T                                  # [n_out, cout]
    val = xj[np.maximum(src, 0), pi[None, :]]
    return np.where(src >= 0, val, np.float32(0))


# ------------------------------------------------------------------------------------------------ (b) probes
@pytest.mark.parametrize("cin,cout,rows,grid", CONV_SHAPES)
def test_conv_selection_probes(dev, cin, cout, rows, grid):
    """centre-tap permutation and tap-dependent selection on a SubM 3x3x3 rulebook, every entry point of the shape,
    classes A-F: the output EQUALS join(split(x)) of the selected input (0 where the rulebook has no neighbour)"""
    from isfusion_amd import spconv as sp
    rb, nbr, K = build_rb(sp, dev, cin + cout, rows, grid)
    assert (nbr < 0).mean() > 0.3 and (nbr[[0, 26]] >= 0).any()
    for kind, taps in (("centre", [13]), ("taps", list(range(K)))):
        w, t, pi = selection_weight(K, cin, cout, cin * 3 + cout, taps)
        p16 = sp.pack_filters_f16x3(T(w.reshape(3, 3, 3, cin, cout), dev))
        for cls in FINITE:
            x = sm.make_class(cls, (rows, cin), 11)
            want = selected(sm.join(*sm.split(x)), nbr, t, pi)
            assert np.array_equal(sm.store_split(want), want)
            xd = T(x, dev)
            names = []
            for name, fn in conv_entries(cin, cout, rb.num_out):
                check_equal(f"conv {cin}->{cout} x{rows} {name} [{kind}]", cls, fn(sp, xd, p16, K, rb, None, None, None, False),
                            want)
                names.append(name)
            report_exact(f"conv {cin}->{cout} x{rows} [{kind}]", cls, " on " + ", ".join(names))


@pytest.mark.parametrize("cin,cout", [(64, 64), (128, 128), (256, 256)])
def test_conv_residual_probe(dev, cin, cout):
    """the residual input of the conv epilogue (join8(res_hi, res_lo)): every tap absent, zero weights, residual = class
    data -> store_split(residual)"""
    from isfusion_amd import spconv as sp
    rows, K = 1000, 27
    stride = _lib.load().isf_nbr_stride(rows)
    rb = sp.Rulebook(torch.full((K, stride), -1, dtype=torch.int32, device=dev), stride, rows, rows, None, None)
    p16 = sp.pack_filters_f16x3(torch.zeros((3, 3, 3, cin, cout), device=dev))
    x = T(sm.make_class("C", (rows, cin), 2), dev)
    # the one-workgroup-per-CU and LDS-staged kernels plan their launch from the rulebook's taps: for them (and once more
    # for the others) the same probe on a real SubM rulebook -- zero weights times finite rows are exact zeros as well
    rb2, _, _ = build_rb(sp, dev, cin, rows, [9, 24, 20])
    absent = [e for e in conv_entries(cin, cout, rows) if e[0].startswith("f16x3 ") or e[0] == "dma"]
    for cls in FINITE:
        res = sm.make_class(cls, (rows, cout), 13)
        for name, fn in absent:
            check_equal(f"conv {cin}->{cout} {name} [residual]", cls, fn(sp, x, p16, K, rb, None, None, T(res, dev), False),
                        sm.store_split(res))
        for name, fn in conv_entries(cin, cout, rows):
            check_equal(f"conv {cin}->{cout} {name} [residual, zero weights]", cls,
                        fn(sp, x, p16, K, rb2, None, None, T(res, dev), False), sm.store_split(res))
        report_exact(f"conv {cin}->{cout} [residual]", cls, " on " + ", ".join(e[0] for e in conv_entries(cin, cout, rows)))


LINEAR_SHAPES = [(700, 256, 256), (1000, 128, 384), (4500, 128, 128), (4500, 64, 384), (4500, 128, 256)]   # (M, K, N)


def permutation_linear(K, N, seed):
    rng = np.random.default_rng([seed, 3])
    pi = np.concatenate([rng.permutation(K) for _ in range((N + K - 1) // K)])[:N]
    w = np.zeros((N, K), np.float32)
    w[np.arange(N), pi] = 1.0
    return w, pi


@pytest.mark.parametrize("M,K,N", LINEAR_SHAPES)
def test_linear_selection_probe(dev, M, K, N):
    """fusion_ops.linear with a permutation weight, no bias: the in-register A-fragment split of isf_linear.hip on the
    64-row tile (M <= 4096 or K = 256) and the 128-row tile (M > 4096, K < 256)"""
    from isfusion_amd import fusion_ops as ops
    w, pi = permutation_linear(K, N, M + N)
    pl = ops.PackedLinear(T(w, dev))
    for cls in FINITE:
        x = sm.make_class(cls, (M, K), 17)
        check_equal(f"linear {M}x{K}->{N}", cls, ops.linear(T(x, dev), pl), sm.join(*sm.split(x))[:, pi])
        report_exact(f"linear {M}x{K}->{N} [permutation]", cls)


SWIN_SHAPES = [(300, 96, 288), (777, 384, 96), (300, 3072, 768)]    # (M, K, N); K = 3072 -> 768 is stage 4's fc2


@pytest.mark.parametrize("M,K,N", SWIN_SHAPES)
def test_swin_gemm_selection_probe(dev, M, K, N):
    """swin.gemm, SWIN_A_ROWS loader without the LayerNorm prologue: the split of isf_swin.hip's A stage"""
    from isfusion_amd import fusion_ops as ops, swin
    w, pi = permutation_linear(K, N, M + K)
    pl = ops.PackedLinear(T(w, dev))
    for cls in FINITE:
        x = sm.make_class(cls, (M, K), 19)
        got = swin.gemm(swin._a(_lib.SWIN_A_ROWS, T(x, dev), ldx=K), M, K, pl)
        check_equal(f"swin.gemm {M}x{K}->{N}", cls, got, sm.join(*sm.split(x))[:, pi])
        report_exact(f"swin.gemm {M}x{K}->{N} [permutation]", cls)


def test_attention_output_side_probe(dev):
    """isf_attention_forward at head dim 16, the P.V side (attn_split4 of V).
    Lk = 1: the softmax is exactly 1 and the output must equal join(split(v)).
    Lk = 513 (a 512-key split, a 1-key split and the merge): one key's score is 400 above the others (q.k / 4 with q = k =
    40 e_0 against zero keys), so every other probability is exp(-400) = 0 in fp32, the row sum is exactly 1 and the merge
    divides by exactly 1: equality here too, no ulp of slack needed."""
    from isfusion_amd import fusion_ops as ops
    heads, E = 8, 128
    for cls in FINITE:
        B, Lq = 64, 50
        v = sm.make_class(cls, (B, E), 23)
        q = T(np.random.default_rng(1).standard_normal((B * Lq, E)).astype(np.float32), dev)
        k = T(np.random.default_rng(2).standard_normal((B, E)).astype(np.float32), dev)
        got = ops.attention(q, k, T(v, dev), B, Lq, 1, E, heads).cpu().numpy().reshape(B, Lq, E)
        want = np.broadcast_to(sm.join(*sm.split(v))[:, None, :], got.shape)
        check_equal("attention hd16 Lk=1", cls, got, want)
        B, Lq, Lk = 6, 40, 513
        dom = np.array([0, 17, 255, 511, 512, 300])              # the dominating key of each batch: both splits, tile edges
        v = sm.make_class(cls, (B * Lk, E), 29)
        kk = np.zeros((B, Lk, E), np.float32)
        kk[np.arange(B), dom, ::16] = 40.0                       # dim 0 of every head
        qq = np.zeros((B * Lq, E), np.float32)
        qq[:, ::16] = 40.0
        got = ops.attention(T(qq, dev), T(kk.reshape(B * Lk, E), dev), T(v, dev), B, Lq, Lk, E, heads).cpu().numpy()
        want = sm.join(*sm.split(v)).reshape(B, Lk, E)[np.arange(B), dom]
        check_equal("attention hd16 Lk=513", cls, got.reshape(B, Lq, E), np.broadcast_to(want[:, None, :], (B, Lq, E)))
        report_exact("attention hd16 Lk=1 and Lk=513 [P.V side]", cls)


# ------------------------------------------------------------------------------------------------ (c) random operands
def conv_weight(K, cin, cout, seed):
    return np.random.default_rng([seed, 21]).normal(0, (1.0 / (6 * cin)) ** 0.5, (K, cin, cout)).astype(np.float32)


def store_error(y):
    return sm.split_bound(y)


def assert_in_domain(y, cls):
    assert np.isfinite(y).all() and np.abs(y).max() < 6e4, (cls, "model output outside the finite domain: bad seed")
    assert np.abs(y).max() > 0


@pytest.mark.parametrize("cin,cout,rows,grid", CONV_SHAPES)
def test_conv_random_operands_componentwise(dev, cin, cout, rows, grid):
    """seeded SubM conv, conv-like weights N(0, 1 / (6 cin)), every entry point of the shape, classes A-E.  Plain:
    E_store = the split store.  BN fold + ReLU variant (classes B, C, E_row): the epilogue is fmaf(acc, scale 2^-sw, shift)
    -- the accumulation error times |scale|, one fp32 rounding of the pre-activation value -- then ReLU (1-Lipschitz)."""
    from isfusion_amd import spconv as sp
    rb, nbr, K = build_rb(sp, dev, cin + cout, rows, grid)
    w = conv_weight(K, cin, cout, cin + 2 * cout)
    p16 = sp.pack_filters_f16x3(T(w.reshape(3, 3, 3, cin, cout), dev))
    rng = np.random.default_rng(cin)
    scale = (rng.random(cout) + 0.5).astype(np.float32)
    for cls in RANDOM:
        x = sm.make_class(cls, (rows, cin), 31)
        y, S, n = sm.conv_model(x, w, nbr, rb.num_out)
        assert_in_domain(y, cls)
        acc = sm.accumulation_bound(S, n)
        xd = T(x, dev)
        for name, fn in conv_entries(cin, cout, rb.num_out):
            check_bound(f"conv {cin}->{cout} x{rows} {name}", cls, fn(sp, xd, p16, K, rb, None, None, None, False), y,
                        acc + store_error(y))
        if cls in ("B", "C", "E_row"):
            shift = (rng.normal(0, 0.2, cout) * min(1.0, float(np.abs(y).max()))).astype(np.float32)
            v = y * scale.astype(np.float64) + shift.astype(np.float64)
            yr = np.maximum(v, 0.0)
            bound = acc * scale + U23 * np.abs(v) + store_error(yr)
            for name, fn in conv_entries(cin, cout, rb.num_out):
                got = fn(sp, xd, p16, K, rb, T(scale, dev), T(shift, dev), None, True)
                check_bound(f"conv {cin}->{cout} x{rows} {name} [BN+ReLU]", cls, got, yr, bound)


@pytest.mark.parametrize("cin,cout", [(64, 64), (128, 128), (128, 256)])
def test_strided_conv_random_operands_componentwise(dev, cin, cout):
    """a stride-2 SparseConv3d rulebook (several inputs per tap column, outputs that are not inputs)"""
    from isfusion_amd import spconv as sp
    rows, grid = 2600, [9, 40, 36]
    rb, nbr, K = build_rb(sp, dev, cin + cout + 1, rows, grid, STRIDED)
    w = conv_weight(K, cin, cout, cin + 3 * cout)
    p16 = sp.pack_filters_f16x3(T(w.reshape(3, 3, 3, cin, cout), dev))
    for cls in RANDOM:
        x = sm.make_class(cls, (rows, cin), 37)
        y, S, n = sm.conv_model(x, w, nbr, rb.num_out)
        assert_in_domain(y, cls)
        for name, fn in conv_entries(cin, cout, rb.num_out):
            check_bound(f"conv s2 {cin}->{cout} {name}", cls, fn(sp, T(x, dev), p16, K, rb, None, None, None, False), y,
                        sm.accumulation_bound(S, n) + store_error(y))


def linear_weight(K, N, seed):
    return np.random.default_rng([seed, 41]).normal(0, (1.0 / (6 * K)) ** 0.5, (N, K)).astype(np.float32)


def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(torch.from_numpy(z / np.sqrt(2.0))).numpy())


def gelu_bound(z, dz):
    """error of 0.5f * z * (1.f + erff(z * 0.70710678f)) evaluated in fp32 on an input off by dz: |gelu'| <= 1.13; the
    erf argument is off by 2 roundings (|x erf'(x)| <= 0.43), erff is accurate to 4 ulp of a value below 1 (the HIP math
    API's documented bound), the sum 1 + erf rounds once: together < 4 * 2^-23 absolute on (1 + erf), times |z| / 2; one
    more rounding for the last product."""
    return 1.13 * dz + 0.5 * np.abs(z) * 4 * U23 + U23 * np.abs(gelu64(z))


@pytest.mark.parametrize("M,K,N", LINEAR_SHAPES)
def test_linear_random_operands_componentwise(dev, M, K, N):
    """fusion_ops.linear: plain (fp32 output: E_store = 0), bias + GELU, bias + residual (the LayerNorm epilogue's input:
    ln=None), and residual + LayerNorm for class C"""
    from isfusion_amd import fusion_ops as ops
    w = linear_weight(K, N, M + K + N)
    rng = np.random.default_rng(N)
    for cls in RANDOM:
        x = sm.make_class(cls, (M, K), 43)
        y, S, n = sm.gemm_model(x, w)
        assert_in_domain(y, cls)
        acc = sm.accumulation_bound(S, n)
        xd = T(x, dev)
        check_bound(f"linear {M}x{K}->{N}", cls, ops.linear(xd, ops.PackedLinear(T(w, dev))).cpu().numpy(), y, acc)
        amp = float(np.abs(y).max())
        b = (rng.normal(0, 0.1, N) * amp).astype(np.float32)
        res = (rng.standard_normal((M, N)) * amp).astype(np.float32)
        z = y + b.astype(np.float64)
        dz = acc + U23 * np.abs(z)
        pl = ops.PackedLinear(T(w, dev), T(b, dev))
        check_bound(f"linear {M}x{K}->{N} [bias+GELU]", cls, ops.linear(xd, pl, act=ops.ACT_GELU).cpu().numpy(), gelu64(z),
                    gelu_bound(z, dz))
        zr = z + res.astype(np.float64)
        pre = ops.linear(xd, pl, residual=T(res, dev)).cpu().numpy()
        check_bound(f"linear {M}x{K}->{N} [bias+residual]", cls, pre, zr, dz + U23 * np.abs(zr))
        if cls == "C" and N <= 256:
            # the LayerNorm epilogue judged on ITS input: the rows the kernel itself produces with ln=None (checked against the
            # model just above), allowed one more rounding each in the fused form -- so the bound holds the LayerNorm's own
            # fp32 evaluation and nothing of the GEMM's slack
            ln = torch.nn.LayerNorm(N)
            ln.weight.data = T((rng.normal(0, 0.2, N) + 1).astype(np.float32), "cpu")
            ln.bias.data = T(rng.normal(0, 0.1, N).astype(np.float32), "cpu")
            g, be = ln.weight.detach().numpy().astype(np.float64), ln.bias.detach().numpy().astype(np.float64)
            got = ops.linear(xd, pl, residual=T(res, dev), ln=ln.to(dev)).cpu().numpy()
            want, bound = sb.layer_norm_bound(pre.astype(np.float64), U23 * np.abs(pre), g, be, ln.eps)
            check_bound(f"linear {M}x{K}->{N} [residual+LN]", cls, got, want, bound)


@pytest.mark.parametrize("M,K,N", SWIN_SHAPES)
def test_swin_gemm_random_operands_componentwise(dev, M, K, N):
    """swin.gemm, plain rows (every class; fp32 output) and with scale / shift / residual"""
    from isfusion_amd import fusion_ops as ops, swin
    w = linear_weight(K, N, M + K)
    pl = ops.PackedLinear(T(w, dev))
    rng = np.random.default_rng(K)
    for cls in RANDOM:
        x = sm.make_class(cls, (M, K), 47)
        y, S, n = sm.gemm_model(x, w)
        assert_in_domain(y, cls)
        acc = sm.accumulation_bound(S, n)
        a = swin._a(_lib.SWIN_A_ROWS, T(x, dev), ldx=K)
        check_bound(f"swin.gemm {M}x{K}->{N}", cls, swin.gemm(a, M, K, pl).cpu().numpy(), y, acc)
        amp = float(np.abs(y).max())
        sc = (rng.random(N) + 0.5).astype(np.float32)
        sh = (rng.normal(0, 0.1, N) * amp).astype(np.float32)
        res = (rng.standard_normal((M, N)) * amp).astype(np.float32)
        v = y * sc.astype(np.float64) + sh.astype(np.float64)
        z = v + res.astype(np.float64)
        got = swin.gemm(a, M, K, pl, scale=T(sc, dev), shift=T(sh, dev), residual=T(res, dev)).cpu().numpy()
        # acc * 2^-sw * scale + shift: <= 2 roundings at the pre-activation value; + residual: one more
        check_bound(f"swin.gemm {M}x{K}->{N} [scale+shift+residual]", cls, got, z,
                    acc * sc + U23 * (np.abs(y * sc) + np.abs(v)) + U23 * np.abs(z))


@pytest.mark.parametrize("M,K,N", [(300, 96, 288), (777, 384, 96)])
def test_swin_gemm_layernorm_prologue_normalises_the_scale_away(dev, M, K, N):
    """with the LN prologue the A operand is (x - mean) rstd gamma + beta: O(1) whatever the input's scale.  Class C against
    the model on the normalised rows; classes A, B and D (the SAME rows times 2^-17 / 2^-9 / 2^12, eps = 0) give the class-C
    result to 1e-5 of its maximum."""
    from isfusion_amd import fusion_ops as ops, swin
    w = linear_weight(K, N, M + K + 7)
    pl = ops.PackedLinear(T(w, dev))
    rng = np.random.default_rng(K + 1)
    g = T((rng.normal(0, 0.2, K) + 1).astype(np.float32), dev)
    b = T(rng.normal(0, 0.1, K).astype(np.float32), dev)
    base = sm.make_class("C", (M, K), 53)
    outs = {}
    for cls, s in (("C", 1.0), ("A", 2.0 ** -17), ("B", 2.0 ** -9), ("D", 2.0 ** 12)):
        xd = T((base * np.float32(s)), dev)
        st = swin.row_stats(swin._a(_lib.SWIN_A_ROWS, xd, ldx=K), M, K, 0.0)
        outs[cls] = swin.gemm(swin._a(_lib.SWIN_A_ROWS, xd, ldx=K, stats=st, ln=(g, b)), M, K, pl).cpu().numpy()
        if cls == "C":
            stn = st.cpu().numpy()
            a = ((base - stn[:, :1]) * stn[:, 1:] * g.cpu().numpy() + b.cpu().numpy()).astype(np.float32)
            y, S, n = sm.gemm_model(a, w)
            # the prologue's four fp32 operations may round differently from numpy's (fused multiply-adds): 4 roundings of
            # an O(|a|) value per element of A, carried through |w|
            slack = 4 * U23 * (np.abs(a).astype(np.float64) + np.abs(b.cpu().numpy())) @ np.abs(w.astype(np.float64)).T
            check_bound(f"swin.gemm {M}x{K}->{N} [LN prologue]", cls, outs[cls], y, sm.accumulation_bound(S, n) + slack)
    top = np.abs(outs["C"]).max()
    for cls in ("A", "B", "D"):
        dev_ = np.abs(outs[cls] - outs["C"]).max() / top
        print(f"split-domain swin.gemm {M}x{K}->{N} [LN prologue] {cls}: max deviation from class C / max = {dev_:.3g}")
        assert dev_ <= 1e-5, (cls, dev_)


@pytest.mark.parametrize("Lk", [200, 700])
def test_attention_random_operands_componentwise(dev, Lk):
    """isf_attention_forward at head dim 16 (Lk = 200: one resident key set; 700: two key splits and the merge) against
    split_blocks.attention_model (the bound is derived there).  O(1) queries and keys with V at classes B, C and D; then the
    probability side at classes A / B (attention_small_probabilities: the output is carried by probabilities of 3e-7 ..
    1.2e-4 alone).  tests/test_split_model.py shows that a flushed V leaves the first bound and flushed probabilities the
    second."""
    from isfusion_amd import fusion_ops as ops
    B, Lq, E, heads = 2, 300, 128, 8
    rng = np.random.default_rng(Lk)
    q = rng.standard_normal((B * Lq, E)).astype(np.float32)
    k = rng.standard_normal((B * Lk, E)).astype(np.float32)
    for cls in ("B", "C", "D"):
        v = sm.make_class(cls, (B * Lk, E), 67)
        y, bound = sb.attention_model(q, k, v, B, Lq, Lk)
        assert_in_domain(y, cls)
        got = ops.attention(T(q, dev), T(k, dev), T(v, dev), B, Lq, Lk, E, heads)
        check_bound(f"attention hd16 Lk={Lk} [QK^T and P.V]", cls, got, y, bound)
    q, k, v = sb.attention_small_probabilities(B, Lq, Lk)
    y, bound = sb.attention_model(q, k, v, B, Lq, Lk)
    assert_in_domain(y, "small P")
    got = ops.attention(T(q, dev), T(k, dev), T(v, dev), B, Lq, Lk, E, heads)
    check_bound(f"attention hd16 Lk={Lk} [P.V]", "probabilities at A / B", got, y, bound)


VFE_CASES = [(True, 255.0, False), (True, 1.0, False), (False, 255.0, False), (False, 1.0, False), (True, 255.0, True),
             (False, 255.0, True)]


@pytest.mark.parametrize("tight,imax,offsets_only", VFE_CASES)
def test_dynamic_vfe_componentwise(dev, oracle_mod, tight, imax, offsets_only):
    """The fused DynamicVFE (isf_vfe.hip: v_cvt_pk_f16_f32 + v_fma_mix conversions of its own) against the DynamicVFE
    forward restated in float64 on the split model (split_blocks.vfe_model, where the bound is derived).  With the seeded
    weights the sums are carried by |xyz| <= 54 and the intensity: that is a closeness check (the bound is ~2e-4 of the
    output) in which the centre / cluster offsets of 1e-4 and below weigh 1e-5 of the output.  offsets_only is the variant in
    which the small operands are judged on their own: layer 1 reads the six offset features alone and neither BN fold has
    a shift, so on the tight cloud every operand of BOTH layers is at class A or B.  tests/test_split_model.py shows that
    a flushed conversion in either layer leaves that variant's bound."""
    lb = sb.vfe_branch(offsets_only)
    pts, coors = sb.vfe_cloud(int(tight) * 2 + int(imax), 1500, tight, imax)
    assert np.array_equal(coors[:, 1:], oracle_mod.dynamic_voxelize(pts, sb.VS, sb.RG))
    f, inv, vc = sb.vfe_features(pts, coors)
    if tight:
        assert np.abs(f[:, -3:]).max() < 1.2e-4 and (np.abs(f[:, -3:]) < 2.0 ** -14).mean() > 0.3
    want, bound = sb.vfe_model(lb, f, inv, len(vc))
    lb = lb.to(dev)
    vf, gvc = lb.pts_voxel_encoder(T(pts, dev), T(coors, dev))
    assert np.array_equal(gvc.cpu().numpy(), vc)
    name = "DynamicVFE (fused, two layers" + (", offset features only)" if offsets_only else ")")
    check_bound(name, f"{'tight' if tight else 'loose'} offsets, intensity <= {imax:g}", vf, want, bound)


WB_CLASSES = [("B", 2.0 ** -9), ("A/B", 2.0 ** -13), ("D", 2.0 ** 12)]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("cls,vs", WB_CLASSES)
def test_window_block_v_classes(dev, cls, vs, shift):
    """isf_window_block_forward (qkv projection + position table, 6 x 6 window attention, out-projection, residual,
    LayerNorm in one kernel; conversion code of its own at four places) with V at class B, at 2^-13 (between A and B: half
    of V has a subnormal hi half) and at class D, each against the SAME layer with V at class C (split_blocks.
    window_block_layer: value rows of in_proj times the power of two vs, out_proj columns times 1 / vs).
      closeness   both outputs against the float64 composition, every stage's bound carried through the next ("full").
                  That bound is class independent slack -- the qkv GEMM's 3 n 2^-24 S through scores and softmax, ~20 % of
                  an output -- and cannot see a conversion fault; it is here to catch a wrong block, not a wrong split.
      class       the two layers share their q / k bits and hand their splits the same V up to the exact factor vs, so the
                  DIFFERENCE of the two outputs is the work of the conversions of V and of the attention output (and of
                  fp32 accumulation noise from P.V on): it must equal the model's difference within
                  window_block_class_tolerance -- 2 split errors of V through P, P.V's and the out-projection's
                  3 n 2^-24 S, 2 split errors of the attention output through |Wo|, the LayerNorm to first order.
                  tests/test_split_model.py shows which flushes leave it."""
    from isfusion_amd import fusion_ops as ops
    B, S, d = sb.WB_B, sb.WB_S, sb.WB_D
    pair = (min(vs, 1.0), max(vs, 1.0))
    x = sb.window_block_input()
    got, model = [], []
    for scale in (1.0, vs):
        layer = sb.window_block_layer(scale, shift, pair)
        model.append(sb.window_block_model(layer, x, shift, vref=model[0]["vj"] * vs if model else None))
        layer = layer.to(dev)
        p_ = ops._encoder_layer_cache(layer, S, 6, shift, 1000.0, dev, B)
        got.append(ops.window_block(T(x, dev), p_["block"], p_["in_bias"], p_["table"], p_["out_bias"], layer.norm1, B, S, d,
                                    8, 6, shift).cpu().numpy().astype(np.float64))
        check_bound(f"window_block S=13 shift={shift} [closeness]", cls if scale == vs else f"C (base of {cls})", got[-1],
                    model[-1]["out"], model[-1]["full"])
    tol = sb.window_block_class_tolerance(*model)
    check_bound(f"window_block S=13 shift={shift} [class {cls} - class C]", cls, got[1] - got[0],
                model[1]["out"] - model[0]["out"], tol)


# ------------------------------------------------------------------------------------------------ (d) overflow
def overflow_report(family, share):
    print(f"split-domain {family} G: non-finite set equals the model's; excluded share {share:.4%}")


@pytest.mark.parametrize("cin,cout,rows,grid", CONV_SHAPES)
def test_conv_overflow_is_loud_and_confined(dev, cin, cout, rows, grid):
    """class G through every conv entry point: the non-finite outputs are exactly the rows that gather a poisoned input row,
    in every column (inf * 0 = NaN); every other output meets the bound of (c).  Second pass with a BN scale of 2^20 on two
    columns: outputs the model puts above 7e4 come back non-finite from the split store, never clamped.  Outputs with
    6e4 <= |model| <= 7e4 are excluded there -- at the f16 overflow threshold (65520) the accumulation error decides which
    side the stored value falls on, the model cannot -- and their share is asserted below 1 %."""
    from isfusion_amd import spconv as sp
    rb, nbr, K = build_rb(sp, dev, cin + cout, rows, grid)
    w = conv_weight(K, cin, cout, cin + 2 * cout)
    p16 = sp.pack_filters_f16x3(T(w.reshape(3, 3, 3, cin, cout), dev))
    x, poisoned = sm.make_overflow((rows, cin), 59, rows=12)
    y, S, n = sm.conv_model(x, w, nbr, rb.num_out)
    bad = np.isnan(y)
    reads = np.isin(nbr, poisoned).any(0)
    assert np.array_equal(bad, np.broadcast_to(reads[:, None], y.shape)) and 0 < reads.sum() < rb.num_out // 4
    assert not ((np.abs(y[~bad]) >= 6e4)).any()
    acc = sm.accumulation_bound(S, n)
    scale = np.ones(cout, np.float32)
    scale[[3, cout - 2]] = 2.0 ** 20
    shift = np.zeros(cout, np.float32)
    v = y * scale.astype(np.float64)
    with np.errstate(invalid="ignore"):
        over, border = np.abs(v) > 7e4, (np.abs(v) >= 6e4) & (np.abs(v) <= 7e4)
    assert over.any() and border.mean() <= 0.01
    xd = T(x, dev)
    for name, fn in conv_entries(cin, cout, rb.num_out):
        got = fn(sp, xd, p16, K, rb, None, None, None, False).cpu().numpy()
        assert np.array_equal(~np.isfinite(got), bad), (name, "non-finite set differs from the model's")
        check_bound(f"conv {cin}->{cout} {name}", "G", np.where(bad, 0, got), np.where(bad, 0, y),
                    np.where(bad, 0, acc + store_error(y)), skip=bad)
        got = fn(sp, xd, p16, K, rb, T(scale, dev), T(shift, dev), None, False).cpu().numpy()
        assert not np.isfinite(got[bad | over]).any(), (name, "an overflowed output came back finite")
        rest = ~(bad | over | border)
        assert np.isfinite(got[rest]).all(), name
        check_bound(f"conv {cin}->{cout} {name} [scale 2^20]", "G", np.where(rest, got, 0), np.where(rest, v, 0),
                    np.where(rest, acc * scale + U23 * np.abs(v) + store_error(v), 0), skip=~rest)
        overflow_report(f"conv {cin}->{cout} {name}", float(border.mean()))


@pytest.mark.parametrize("family", ["linear", "swin.gemm"])
def test_gemm_overflow_is_loud_and_confined(dev, family):
    """class G through fusion_ops.linear and swin.gemm (fp32 outputs: nothing overflows on the way out): the non-finite
    outputs are exactly the poisoned rows, whole rows; nothing is excluded"""
    from isfusion_amd import fusion_ops as ops, swin
    for M, K, N in (LINEAR_SHAPES if family == "linear" else SWIN_SHAPES):
        w = linear_weight(K, N, M + K + N)
        w[:, ::3] = 0                                   # inf * 0
        pl = ops.PackedLinear(T(w, dev))
        x, poisoned = sm.make_overflow((M, K), 61, rows=12)
        y, S, n = sm.gemm_model(x, w)
        bad = np.isnan(y)
        assert np.array_equal(np.flatnonzero(bad.all(1)), poisoned) and bad.sum() == poisoned.size * N
        if family == "linear":
            got = ops.linear(T(x, dev), pl).cpu().numpy()
        else:
            got = swin.gemm(swin._a(_lib.SWIN_A_ROWS, T(x, dev), ldx=K), M, K, pl).cpu().numpy()
        assert np.array_equal(~np.isfinite(got), bad), (family, M, K, N)
        check_bound(f"{family} {M}x{K}->{N}", "G", np.where(bad, 0, got), np.where(bad, 0, y),
                    np.where(bad, 0, sm.accumulation_bound(S, n)), skip=bad)
        overflow_report(f"{family} {M}x{K}->{N}", 0.0)
