"""GPU tests of the camera backbone's f16 inference mode (isf_swin_gemm_f16, isf_swin_window_attention_f16,
isf_pack_linear_f16, SwinTransformer.set_precision, ISFusionDetector.camera_precision).

Kernels are compared with float64 torch on the SAME f16-rounded operands, so what is left is the arithmetic of the
kernel itself; each bound is worked out from the number formats next to the test that uses it.  Whole modules are
compared with the float64 restatement (tests/camera_common.py) under the rule

    err_hip <= 2 * err_autocast + 2^-11 * max|ref|          (err = max |x - ref64|)

where err_autocast is the error of the same restatement with fp32 weights under torch.autocast("cuda", float16) on the
same GPU -- what the stock stack computes in the reference's fp16 mode -- and the floor is one f16 rounding of the
largest entry.  The guard err_autocast <= 1e-2 * max|ref| keeps a comparison from passing on ill-conditioned inputs
(tests/test_camera_f16.py shows it on the CPU for the backbone cases)."""
import ast
import os

import pytest
import torch
import torch.nn.functional as F

import camera_common as CC
from test_camera import BACKBONE_SEED, NECK_SEED
from test_camera_f16 import BACKBONE_CASES

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
U16 = 2.0 ** -11          # unit roundoff of f16
U32 = 2.0 ** -24


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return lambda *shape, s=1.0: (torch.randn(*shape, generator=g, dtype=torch.float64) * s).to(DEV)


def _err(a, ref):
    return float((a.detach().double() - ref).abs().max())


def _rule(what, got, ref, ac):
    """the module-level rule and its guard; prints the figures"""
    e_hip, e_ac, top = _err(got, ref), _err(ac, ref), float(ref.abs().max())
    bound = 2 * e_ac + U16 * top
    print(f"{what}: err_hip {e_hip:.3e}  err_autocast {e_ac:.3e}  bound {bound:.3e}  max|ref| {top:.3e}")
    assert e_ac <= 1e-2 * top, (what, e_ac, top)
    assert e_hip <= bound, (what, e_hip, bound)


# ---------------------------------------------------------------------------------------------- window attention
def _attention_ref(qkv, bias, table, B, H, W, C, heads, shift):
    """float64: padded cells carry qkv = bias (zero input after norm1), roll, windows, masked softmax, reverse, crop"""
    Hp, Wp = -(-H // 7) * 7, -(-W // 7) * 7
    pad = bias if bias is not None else torch.zeros(3 * C, dtype=torch.float64, device=DEV)
    grid = pad.expand(B, Hp, Wp, 3 * C).clone()
    grid[:, :H, :W] = qkv.view(B, H, W, 3 * C)
    if shift:
        grid = torch.roll(grid, (-shift, -shift), (1, 2))
    win = CC._windows(grid, 7)
    q, k, v = win.view(-1, 49, 3, heads, 32).permute(2, 0, 3, 1, 4)
    att = (q * 32 ** -0.5) @ k.transpose(-2, -1) + table[None]
    if shift:
        lab = torch.zeros(1, Hp, Wp, 1, dtype=torch.float64, device=DEV)
        sl = (slice(0, -7), slice(-7, -shift), slice(-shift, None))
        for i, a in enumerate(sl):
            for j, b in enumerate(sl):
                lab[:, a, b] = 3 * i + j
        mw = CC._windows(lab, 7).squeeze(-1)
        m = (mw[:, None, :] != mw[:, :, None]).double() * -100.0
        att = att + m.repeat(B, 1, 1)[:, None]
    o = (att.softmax(-1) @ v).transpose(1, 2).reshape(-1, 49, C)
    o = CC._unwindows(o, B, Hp, Wp, 7)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    return o[:, :H, :W].reshape(B * H * W, C)


def _attention_case(C, heads, H, W, shift, with_bias, seed):
    """Bound: the kernel's scores and softmax are fp32 (relative error of a probability ~ |s| 2^-23 + expf < 4e-5 for
    |s| <= 100 + a few), each probability is rounded to f16 once (weights sum to 1 in fp32, so the rounding moves the
    output by at most 2^-11 max|v|) and the output is rounded to f16 once (<= 2^-11 max|v|):
    err <= (2^-10 + 4e-5) * max|v| over the value third of qkv and the bias."""
    from isfusion_amd import swin
    r = _gen(seed)
    B = 2
    qkv16 = r(B * H * W, 3 * C).half()
    bias = r(3 * C, s=0.5).float() if with_bias else None
    table = r(heads, 49, 49, s=0.5).float()
    got = swin.window_attention(qkv16, bias, table, B, H, W, C, heads, 7, shift, 32 ** -0.5)
    assert got.dtype == torch.float16 and tuple(got.shape) == (B * H * W, C)
    b64 = None if bias is None else bias.half().double()          # a padded cell holds the bias as the qkv GEMM stores it
    ref = _attention_ref(qkv16.double(), b64, table.double(), B, H, W, C, heads, shift)
    vmax = float(qkv16[:, 2 * C:].abs().max())
    if b64 is not None:
        vmax = max(vmax, float(b64[2 * C:].abs().max()))
    bound = (2 * U16 + 4e-5) * vmax
    e = _err(got, ref)
    print(f"attention C {C} grid {H}x{W} shift {shift} bias {with_bias}: err {e:.3e}  bound {bound:.3e}")
    assert e <= bound, (e, bound)


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("grid", [(14, 21), (9, 10), (5, 9)])
@pytest.mark.parametrize("ch", [(96, 3), (768, 24)])
def test_window_attention_f16_equals_float64(ch, grid, shift):
    """(14, 21): whole windows only; (9, 10): padding on both axes; (5, 9): a grid smaller than one window in H"""
    _attention_case(ch[0], ch[1], grid[0], grid[1], shift, True, 7 * grid[0] + grid[1] + shift + ch[1])


def test_window_attention_f16_without_qkv_bias():
    _attention_case(96, 3, 9, 10, 3, False, 5)


# --------------------------------------------------------------------------------------------------- GEMM forms
def _gemm_bound(a16, w16, ref, K, a_rounded_in_kernel, y16, gelu):
    """|sum a w| over exact f16 products accumulated in fp32: <= K 2^-24 S, S = max over outputs of sum |a| |w|.  When the
    kernel rounds fp32 A values that differ from the reference's (LayerNorm computed in fp32, the reference's in
    float64), an element may round to the neighbouring f16: one f16 rounding of A, <= 2^-11 S.  GELU's slope is <= 1.13.
    An f16 output adds one rounding of the result."""
    S = float((a16.abs() @ w16.abs().t()).max())
    b = (K * U32 + (U16 if a_rounded_in_kernel else 0.0)) * S * (1.13 if gelu else 1.0)
    return b + (U16 * float(ref.abs().max()) if y16 else 0.0)


@pytest.mark.parametrize("shape", [(130, 96, 384), (257, 192, 96)])
def test_rows_layernorm_gelu_f16_out_equals_float64(shape):
    """ROWS + LayerNorm prologue -> f16 out with GELU (norm2 + fc1 of the f16 block).
    M = 130 / 257: not multiples of the 128-row tile; N = 96: one and a half 64-column tiles"""
    from isfusion_amd import _lib, swin
    from isfusion_amd.fusion_ops import ACT_GELU
    M, K, N = shape
    r = _gen(M + K + N)
    x, g, b = (r(M, K, s=3.0) + 0.5).float(), (1 + r(K, s=0.1)).float(), r(K, s=0.1).float()
    w, bias = r(N, K, s=K ** -0.5).float(), r(N, s=0.1).float()
    st = swin.row_stats(swin._a(_lib.SWIN_A_ROWS, x, ldx=K), M, K, 1e-5)
    got = swin.gemm(swin._a(_lib.SWIN_A_ROWS, x, ldx=K, stats=st, ln=(g, b)), M, K, swin.PackedLinearF16(w),
                    shift=bias, act=ACT_GELU, out_f16=True)
    assert got.dtype == torch.float16
    a16 = F.layer_norm(x.double(), (K,), g.double(), b.double(), 1e-5).half().double()
    w16 = w.half().double()
    ref = F.gelu(a16 @ w16.t() + bias.double())
    bound = _gemm_bound(a16, w16, ref, K, True, True, True)
    e = _err(got, ref)
    print(f"rows+LN+GELU -> f16 {shape}: err {e:.3e}  bound {bound:.3e}")
    assert e <= bound, (e, bound)


def test_rows_f16_in_fp32_out_bias_residual_equals_float64():
    from isfusion_amd import _lib, swin
    M, K, N = 130, 3072, 768
    r = _gen(31)
    h16 = r(M, K).half()
    w, bias, res = r(N, K, s=K ** -0.5).float(), r(N, s=0.1).float(), r(M, N).float()
    got = swin.gemm(swin._a(_lib.SWIN_A_ROWS, h16, ldx=K), M, K, swin.PackedLinearF16(w), shift=bias, residual=res)
    assert got.dtype == torch.float32
    w16 = w.half().double()
    ref = h16.double() @ w16.t() + bias.double() + res.double()
    bound = _gemm_bound(h16.double(), w16, ref, K, False, False, False) + 2 * U32 * float(ref.abs().max())
    e = _err(got, ref)
    print(f"rows f16 -> fp32 K {K}: err {e:.3e}  bound {bound:.3e}")
    assert e <= bound, (e, bound)


@pytest.mark.parametrize("grid", [(23, 33, 96), (5, 9, 384)])
def test_patch_merging_f16_equals_float64(grid):
    """odd grids: corner padding; the packed weight and gamma / beta carry the loader's (kh*2 + kw)*C + c order"""
    from isfusion_amd.swin import PackedLinearF16, PatchMerging
    H, W, C = grid
    B = 2
    r = _gen(H + W + C)
    m = PatchMerging(C, 2 * C).to(DEV).eval()
    with torch.no_grad():
        m.norm.weight.copy_(1 + r(4 * C, s=0.1))
        m.norm.bias.copy_(r(4 * C, s=0.1))
        m.reduction.weight.copy_(r(2 * C, 4 * C, s=(4 * C) ** -0.5))
    x = r(B * H * W, C, s=2.0).float()
    got, (Ho, Wo) = m.run(m.pack(PackedLinearF16), x, B, H, W)
    assert got.dtype == torch.float32
    xm = x.double().view(B, H, W, C).permute(0, 3, 1, 2)
    xm = F.unfold(F.pad(xm, (0, W % 2, 0, H % 2)), kernel_size=2, stride=2).transpose(1, 2)
    a16 = F.layer_norm(xm, (4 * C,), m.norm.weight.double(), m.norm.bias.double(), 1e-5).half().double()
    w16 = m.reduction.weight.detach().half().double()
    ref = a16 @ w16.t()
    assert (Ho, Wo) == ((H + 1) // 2, (W + 1) // 2)
    bound = _gemm_bound(a16.reshape(-1, 4 * C), w16, ref, 4 * C, True, False, False)
    e = _err(got.view(ref.shape), ref)
    print(f"merge {grid}: err {e:.3e}  bound {bound:.3e}")
    assert e <= bound, (e, bound)


@pytest.mark.parametrize("hw", [(33, 46), (90, 150)])
def test_patch_gemm_f16_equals_float64(hw):
    """the 4 x 4 patch conv before PatchEmbed's LayerNorm: the image is rounded to f16 by the loader exactly as
    .half() rounds it, so only the fp32 accumulation is left"""
    from isfusion_amd import _lib, swin
    H, W = hw
    r = _gen(H * W)
    m = swin.PatchEmbed(3, 96, 4, 4, dict(type="LN")).to(DEV).eval()
    with torch.no_grad():
        m.projection.weight.copy_(r(96, 3, 4, 4, s=0.15))
        m.projection.bias.copy_(r(96, s=0.1))
    img = r(2, 3, H, W).float()
    p = m.pack(swin.PackedLinearF16)
    Ho, Wo = (H + 3) // 4, (W + 3) // 4
    got = swin.gemm(swin._a(_lib.SWIN_A_PATCH, img, n=2, c=3, h=H, w=W), 2 * Ho * Wo, p["k"], p["w"], shift=p["b"])
    i16 = F.pad(img.half().double(), (0, (-W) % 4, 0, (-H) % 4))
    w16 = m.projection.weight.detach().half().double()
    ref = F.conv2d(i16, w16, m.projection.bias.double(), stride=4).flatten(2).transpose(1, 2).reshape(-1, 96)
    a16 = F.unfold(i16, kernel_size=4, stride=4).transpose(1, 2).reshape(-1, 48)
    bound = _gemm_bound(a16, w16.flatten(1), ref, 64, False, False, False) + 2 * U32 * float(ref.abs().max())
    e = _err(got, ref)
    print(f"patch {hw}: err {e:.3e}  bound {bound:.3e}")
    assert e <= bound, (e, bound)
    # and the module's run() in this mode: the same rows through the fp32 LayerNorm pass
    with torch.no_grad():
        m.norm.weight.copy_(1 + r(96, s=0.1))
        m.norm.bias.copy_(r(96, s=0.1))
    rows, ghw = m.run(p, img)
    assert ghw == (Ho, Wo)
    assert torch.equal(rows, swin.layernorm(got, m.norm))


def test_layernorm_prologue_f16_is_exact_in_every_round_of_workgroups():
    """ROWS + LayerNorm prologue and MERGE + LayerNorm prologue at 12 x 96 x 264 tokens: 2376 / 594 row tiles, several
    rounds of workgroups per compute unit.  The vector form of the prologue's arithmetic lost the normalised term of
    single elements in later rounds; every output is checked, twice, and the two runs compared bit for
    bit.  Bound as in the small cases (fp32 output)."""
    from isfusion_amd import _lib, swin
    from isfusion_amd.swin import PackedLinearF16, PatchMerging
    B, H, W, C, N = 12, 96, 264, 96, 288
    M = B * H * W
    r = _gen(77)
    x, g, b = (r(M, C, s=3.0) + 0.5).float(), (1 + r(C, s=0.1)).float(), r(C, s=0.1).float()
    w = r(N, C, s=C ** -0.5).float()
    pl = PackedLinearF16(w)
    st = swin.row_stats(swin._a(_lib.SWIN_A_ROWS, x, ldx=C), M, C, 1e-5)
    runs = [swin.gemm(swin._a(_lib.SWIN_A_ROWS, x, ldx=C, stats=st, ln=(g, b)), M, C, pl) for _ in range(2)]
    a16 = F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-5).half().double()
    w16 = w.half().double()
    ref = a16 @ w16.t()
    bound = _gemm_bound(a16, w16, ref, C, True, False, False)
    e = _err(runs[0], ref)
    print(f"rows+LN at {M} rows: err {e:.3e}  bound {bound:.3e}")
    assert torch.equal(runs[0], runs[1]) and e <= bound, (e, bound)
    m = PatchMerging(C, 2 * C).to(DEV).eval()
    m.load_state_dict(CC.seeded_module_state(m, 5))
    p = m.pack(PackedLinearF16)
    got, again = m.run(p, x, B, H, W)[0], m.run(p, x, B, H, W)[0]
    sd = {"m." + k: v.double() for k, v in m.state_dict().items()}
    xm = x.double().view(B, H, W, C).permute(0, 3, 1, 2)
    xm = F.unfold(xm, kernel_size=2, stride=2).transpose(1, 2)
    a16 = F.layer_norm(xm, (4 * C,), sd["m.norm.weight"], sd["m.norm.bias"], 1e-5).half().double().reshape(-1, 4 * C)
    w16 = m.reduction.weight.detach().half().double()
    ref = a16 @ w16.t()
    bound = _gemm_bound(a16, w16, ref, 4 * C, True, False, False)
    e = _err(got, ref)
    print(f"merge+LN at {a16.shape[0]} rows: err {e:.3e}  bound {bound:.3e}")
    assert torch.equal(got, again) and e <= bound, (e, bound)


def test_block_f16_is_bit_identical_run_to_run_at_full_size():
    """one stage-0 block at 12 x 96 x 264 tokens (2376 row tiles: several rounds of workgroups per compute unit)"""
    from isfusion_amd.swin import PackedLinearF16, SwinBlock
    blk = SwinBlock(96, 3, 384, shift=True).to(DEV).eval()
    blk.load_state_dict(CC.seeded_module_state(blk, 21))
    B, H, W = 12, 96, 264
    x = _gen(8)(B * H * W, 96).float()
    p = blk.pack(PackedLinearF16)
    a, b = blk.run(p, x, B, H, W), blk.run(p, x, B, H, W)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    sd64 = CC.cast({"b." + k: v for k, v in blk.state_dict().items()}, torch.float64, DEV)
    sd32 = CC.cast({"b." + k: v for k, v in blk.state_dict().items()}, torch.float32, DEV)
    with torch.no_grad():
        ref = CC.swin_block(sd64, "b.", x.double().view(B, H * W, 96), (H, W), 3, 7, 3).reshape(-1, 96)
        with torch.autocast("cuda", dtype=torch.float16):
            ac = CC.swin_block(sd32, "b.", x.view(B, H * W, 96), (H, W), 3, 7, 3).reshape(-1, 96)
    _rule("stage-0 block at 12 x 96 x 264", a, ref, ac)


def test_gemm_forms_that_are_not_built_are_refused_before_a_launch():
    """the launcher's table of built forms (swin_gemm_forms): every combination outside it, and a null row_scale, comes
    back with a code and a message, and y keeps its fill.  Arguments are valid otherwise, so the loader checks pass."""
    import ctypes
    from isfusion_amd import _lib, swin
    from isfusion_amd.fusion_ops import PackedLinear
    lib = _lib.load()
    M, K, N = 16, 32, 16
    r = _gen(41)
    w = r(N, K).float()
    x3, f16 = PackedLinear(w), swin.PackedLinearF16(w)
    x, g, b = r(M, K).float(), r(K).float(), r(K).float()
    st = swin.row_stats(swin._a(_lib.SWIN_A_ROWS, x, ldx=K), M, K, 1e-5)
    rows = swin._a(_lib.SWIN_A_ROWS, x, ldx=K)
    rows_ln = swin._a(_lib.SWIN_A_ROWS, x, ldx=K, stats=st, ln=(g, b))
    rows16_ln = swin._a(_lib.SWIN_A_ROWS, x.half(), ldx=K, stats=st, ln=(g, b))
    merge = swin._a(_lib.SWIN_A_MERGE, r(64, 8).float(), n=1, c=8, h=8, w=8)
    upcat = swin._a(_lib.SWIN_A_UPCAT, r(1, 16, 4, 4).float(), n=1, c=16, h=4, w=4, x2=r(1, 16, 2, 2).float(), c2=16,
                    h2=2, w2=2)
    keep = torch.ones(1, dtype=torch.float32, device=DEV)
    y = torch.full((M, N), 7.0, dtype=torch.float32, device=DEV)
    yp, stream = _lib.ptr(y), _lib.stream()

    def gemm_f16(a, a16, pl, y16, y_hw):
        return lib.isf_swin_gemm_f16(ctypes.byref(a[0]), a16, M, K, _lib.ptr(pl.packed), N, None, None, 0, None, yp, y16,
                                     0 if y_hw else N, y_hw, stream)

    def gemm_rowscale(a, row_scale):
        return lib.isf_swin_gemm_rowscale(ctypes.byref(a[0]), M, K, _lib.ptr(x3.packed), N, None, None, 0, None,
                                          _lib.ptr(row_scale), M, yp, N, 0, stream)

    cases = {"f16 mode, UPCAT loader": lambda: gemm_f16(upcat, 0, f16, 0, 0),
             "f16 mode, y_hw > 0": lambda: gemm_f16(rows, 0, f16, 0, M),
             "f16 A rows, LayerNorm prologue": lambda: gemm_f16(rows16_ln, 1, f16, 0, 0),
             "f16 output, MERGE loader": lambda: gemm_f16(merge, 0, f16, 1, 0),
             "row scale, LayerNorm prologue": lambda: gemm_rowscale(rows_ln, keep),
             "isf_swin_gemm_rowscale, null row_scale": lambda: gemm_rowscale(rows, None)}
    for what, call in cases.items():
        rc = call()
        msg = lib.isf_last_error().decode()
        print(f"{what}: code {rc}, {msg!r}")
        assert rc != _lib.ISF_OK and msg.startswith("swin_gemm"), (what, rc, msg)
    assert bool((y == 7.0).all())
    with pytest.raises(NotImplementedError, match="row_scale"):
        swin.gemm(rows, M, K, f16, row_scale=keep)
    assert gemm_f16(rows, 0, f16, 0, 0) == _lib.ISF_OK and not bool((y == 7.0).any())     # the calls above were valid


# --------------------------------------------------------------------------------------------------- backbone
def _backbone(seed=BACKBONE_SEED, dev=DEV):
    from test_camera import _modules
    bb, _ = _modules()
    bb.load_state_dict(CC.seeded_module_state(bb, seed))
    return bb.to(dev).eval()


def _autocast_swin(sd32, img):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        return CC.swin_forward(sd32, img)


@pytest.mark.parametrize("case", range(len(BACKBONE_CASES)))
def test_backbone_f16_meets_the_rule(case):
    n, h, w, seed = BACKBONE_CASES[case]
    bb = _backbone().set_precision("f16")
    img = CC.images(seed, n, h, w).to(DEV)
    got = bb(img)
    with torch.no_grad():
        ref = CC.swin_forward(CC.cast(bb.state_dict(), torch.float64, DEV), img.double())
    ac = _autocast_swin(CC.cast(bb.state_dict(), torch.float32, DEV), img)
    assert len(got) == 3
    for li, (a, b, c) in enumerate(zip(got, ref, ac)):
        assert a.dtype == torch.float32 and tuple(a.shape) == tuple(b.shape)
        _rule(f"backbone {n}x{h}x{w} map {li}", a, b, c)


def test_modes_do_not_leak():
    img = CC.images(101, 1, 90, 150).to(DEV)
    bb = _backbone()
    first = bb(img)
    bb.set_precision("f16")
    h1 = bb(img)
    h2 = bb(img)
    bb.set_precision("f32")
    back = bb(img)
    fresh = _backbone()(img)
    for a, b, c in zip(first, back, fresh):
        assert torch.equal(a, c) and torch.equal(b, c)                  # f32 -> f16 -> f32 == never left f32
    for a, b in zip(h1, h2):
        assert torch.equal(a, b)                                        # f16 is bit-identical run to run
    assert not torch.equal(h1[0], first[0])                             # and really another arithmetic
    # new weights while in f16 mode: the packed copies are re-derived through the cache
    bb.set_precision("f16")
    other = CC.seeded_module_state(bb, BACKBONE_SEED + 1)
    bb.load_state_dict(other, strict=True)
    reloaded = bb(img)
    want = _backbone(BACKBONE_SEED + 1).set_precision("f16")(img)
    for a, b, c in zip(reloaded, want, h1):
        assert torch.equal(a, b) and not torch.equal(a, c)


def test_f16_stores_saturate():
    """one C = 96 block whose fc1 weights are scaled until the FFN hidden passes the f16 range: stored as +-65504, not
    inf, so every output stays finite"""
    from isfusion_amd.swin import PackedLinearF16, SwinBlock
    r = _gen(3)
    blk = SwinBlock(96, 3, 384).to(DEV).eval()
    sd = CC.seeded_module_state(blk, 12)
    sd["ffn.layers.0.0.weight"] = sd["ffn.layers.0.0.weight"] * 1e6
    blk.load_state_dict(sd)
    B, H, W = 2, 9, 10
    x = r(B * H * W, 96).float()
    y = blk.run(blk.pack(PackedLinearF16), x, B, H, W)
    # the premise, in float64: the hidden does leave the f16 range
    sd64 = CC.cast({"b." + k: v for k, v in blk.state_dict().items()}, torch.float64, DEV)
    x64 = x.double().view(B, H * W, 96)
    y1 = x64 + CC.shift_window_msa(sd64, "b.attn.", CC._ln(sd64, "b.norm1.", x64), (H, W), 3, 7, 0)
    hid = F.gelu(F.linear(CC._ln(sd64, "b.norm2.", y1), sd64["b.ffn.layers.0.0.weight"], sd64["b.ffn.layers.0.0.bias"]))
    assert float(hid.max()) > 65504.0
    assert y.dtype == torch.float32 and bool(torch.isfinite(y).all())
    # the saturated hidden is 65504 where the true one is larger: |fc2 output| <= 65504 * sum |w| + |bias| + |y1|
    w2 = sd64["b.ffn.layers.1.weight"]
    cap = 65504.0 * float(w2.abs().sum(1).max()) + float(sd64["b.ffn.layers.1.bias"].abs().max()) + float(y1.abs().max())
    assert float(y.abs().max()) <= 1.01 * cap


# --------------------------------------------------------------------------------------------------- detector
_DET = {}


def _detector():
    if "det" not in _DET:
        from detector_common import build_path, detector_inputs
        from isfusion_amd import registry
        from test_camera import _modules
        with open(os.path.join(HERE, "golden", "isfusion_0075voxel_model.txt")) as f:
            model = ast.literal_eval(f.read())
        path = build_path()
        bb, nk = _modules()
        bb.load_state_dict(CC.seeded_module_state(bb, BACKBONE_SEED))
        nk.load_state_dict(CC.seeded_module_state(nk, NECK_SEED))
        det = registry.build_detector({"model": model})
        sd = dict(path.state_dict())
        sd.update({"img_backbone." + k: v for k, v in bb.state_dict().items()})
        sd.update({"img_neck." + k: v for k, v in nk.state_dict().items()})
        det.load_state_dict(sd, strict=True)
        _DET["det"] = det.to(DEV).eval()
        pts, inp, kw, metas = detector_inputs()
        img = CC.images(11, 6 * len(pts), 384, 1056).view(len(pts), 6, 3, 384, 1056).to(DEV)
        _DET["inputs"] = ([torch.from_numpy(p).to(DEV) for p in pts], img, kw, metas)
    return _DET["det"], _DET["inputs"]


def test_detector_camera_precision_f16():
    det, (pts, img, kw, metas) = _detector()
    det.camera_precision = "f16"
    try:
        assert det.img_backbone.precision == "f16"
        got = det.extract_img_feat(img.clone(), [dict(m) for m in metas])      # packs the weights
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            again = det.extract_img_feat(img.clone(), [dict(m) for m in metas])
        finally:
            torch.cuda.set_sync_debug_mode(0)
        for a, b in zip(got, again):
            assert torch.equal(a, b)
        flat = img.view(-1, 3, 384, 1056)
        bsd, nsd = det.img_backbone.state_dict(), det.img_neck.state_dict()
        with torch.no_grad():
            ref = CC.neck_forward(CC.cast(nsd, torch.float64, DEV),
                                  CC.swin_forward(CC.cast(bsd, torch.float64, DEV), flat.double()))
            with torch.autocast("cuda", dtype=torch.float16):
                ac = CC.neck_forward(CC.cast(nsd, torch.float32, DEV),
                                     CC.swin_forward(CC.cast(bsd, torch.float32, DEV), flat))
        assert len(got) == len(ref) == 2
        for li, (a, b, c) in enumerate(zip(got, ref, ac)):
            _rule(f"extract_img_feat level {li}", a, b, c)
        res = det.simple_test(pts, [dict(m) for m in metas], img=img.clone(), **kw)
        assert len(res) == len(pts)
        for one in res:
            box = one["pts_bbox"]
            assert set(box) >= {"boxes_3d", "scores_3d", "labels_3d"}
            assert box["scores_3d"].shape[0] == box["labels_3d"].shape[0] == box["boxes_3d"].shape[0]
    finally:
        det.camera_precision = "f32"
