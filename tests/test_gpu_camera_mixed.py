"""GPU tests of the camera backbone's mixed-precision training mode (isf_swin_gemm_f16_rowscale,
isf_rows_weight_grad_f16, isf_swin_window_attention_backward_f16, SwinTransformer.set_precision("mixed"),
ISFusionDetector.camera_precision = "mixed").

Single products (the row-scale GEMM, dW) are compared with float64 on the SAME f16-rounded operands, so what is left is
the kernel's own arithmetic; the bound is worked out from the number formats next to each test.  The attention backward
and whole modules are compared with the float64 restatement under the f16 inference mode's rule
(tests/camera_mixed_common.py): err_hip <= 2 * err_autocast + 2^-11 * max|ref|, err_autocast being the error of the same
restatement with fp32 leaves under torch.autocast("cuda", float16), forward and backward, on the same GPU."""
import pytest
import torch

import camera_common as CC
import camera_mixed_common as CM
import camera_train_common as CT
import test_gpu_camera_train as G
from test_gpu_camera_f16 import _gemm_bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_gen = G._gen
U32 = 2.0 ** -24
ROWS, PARAMS = CM.GUARD_ROWS, CM.GUARD_PARAMS


# ------------------------------------------------------------------------------------------- 1. f16 row-scale GEMM
@pytest.mark.parametrize("shape", [(3, 5, 7, 96, 96), (3, 5, 7, 384, 96), (2, 9, 15, 96, 96)])
def test_gemm_f16_rowscale_equals_float64(shape):
    """105 rows: three samples inside one 128-row tile; 270 rows: a sample boundary inside a tile.  Bound: _gemm_bound
    (exact f16 products, fp32 accumulation) + two fp32 roundings of the result (the factor, the residual add)."""
    from isfusion_amd import _lib, swin
    B, H, W, K, N = shape
    M = B * H * W
    r = _gen(B * H * W + K)
    a16 = r(M, K).half()
    w, b, res = r(N, K, s=K ** -0.5).float(), r(N, s=0.1).float(), r(M, N).float()
    scale = torch.tensor([1 / 0.8, 0.0, 1 / 0.8][:B], dtype=torch.float32, device=DEV)
    pl = swin.PackedLinearF16(w)
    rows = lambda: swin._a(_lib.SWIN_A_ROWS, a16, ldx=K)
    got = swin.gemm_f16_rowscale(rows(), M, K, pl, scale, shift=b, residual=res)
    assert got.dtype == torch.float32
    w16 = w.half().double()
    per_row = scale.double().repeat_interleave(H * W)[:, None]
    ref = (a16.double() @ w16.t() + b.double()) * per_row + res.double()
    bound = _gemm_bound(a16.double(), w16, ref, K, False, False, False) + 2 * U32 * float(ref.abs().max())
    e = float((got.double() - ref).abs().max())
    print(f"f16 rowscale {shape}: err {e:.3e}  bound {bound:.3e}")
    assert e <= bound, (e, bound)
    dropped = (per_row == 0).expand_as(ref)
    assert dropped.any() and torch.equal(got[dropped], res[dropped])          # bit for bit the residual
    ones = torch.ones(B, dtype=torch.float32, device=DEV)
    plain = swin.gemm(rows(), M, K, pl, shift=b, residual=res)
    assert torch.equal(swin.gemm_f16_rowscale(rows(), M, K, pl, ones, shift=b, residual=res), plain)
    # through the block's dispatch: the f16 pack with a factor goes to the new entry, gemm itself keeps refusing it
    assert torch.equal(swin._branch_out(rows(), M, K, pl, b, res, scale), got)
    with pytest.raises(NotImplementedError, match="row_scale"):
        swin.gemm(rows(), M, K, pl, row_scale=scale)


def test_gemm_f16_rowscale_refuses_what_is_not_built():
    import ctypes
    from isfusion_amd import _lib, swin
    lib = _lib.load()
    M, K, N = 16, 32, 16
    r = _gen(43)
    f16 = swin.PackedLinearF16(r(N, K).float())
    x, g, b = r(M, K).float(), r(K).float(), r(K).float()
    st = swin.row_stats(swin._a(_lib.SWIN_A_ROWS, x, ldx=K), M, K, 1e-5)
    rows16 = swin._a(_lib.SWIN_A_ROWS, x.half(), ldx=K)
    rows32_ln = swin._a(_lib.SWIN_A_ROWS, x, ldx=K, stats=st, ln=(g, b))
    keep = torch.ones(1, dtype=torch.float32, device=DEV)
    y = torch.full((M, N), 7.0, dtype=torch.float32, device=DEV)

    def call(a, a16, row_scale, y16=0):
        return lib.isf_swin_gemm_f16_rowscale(ctypes.byref(a[0]), a16, M, K, _lib.ptr(f16.packed), N, None, None, 0, None,
                                              _lib.ptr(row_scale), M, _lib.ptr(y), y16, N, 0, _lib.stream())

    cases = {"null row_scale": lambda: call(rows16, 1, None),
             "LayerNorm prologue": lambda: call(rows32_ln, 0, keep),
             "fp32 A rows": lambda: call(swin._a(_lib.SWIN_A_ROWS, x, ldx=K), 0, keep),
             "f16 output": lambda: call(rows16, 1, keep, 1)}
    for what, c in cases.items():
        rc = c()
        msg = lib.isf_last_error().decode()
        print(f"{what}: code {rc}, {msg!r}")
        assert rc != _lib.ISF_OK and msg.startswith("swin_gemm"), (what, rc, msg)
    assert bool((y == 7.0).all())
    assert call(rows16, 1, keep) == _lib.ISF_OK and not bool((y == 7.0).any())        # the calls above were valid


# ---------------------------------------------------------------------------------------------- 2. single-pass dW
@pytest.mark.parametrize("x16", [False, True])
@pytest.mark.parametrize("R,N,K", [(105, 96, 96), (130, 288, 96), (1000, 384, 1536)])
def test_rows_weight_grad_f16_equals_float64(R, N, K, x16):
    """(105, 96, 96): four one-step chunks with a ragged last step, N and K no multiples of the 128 x 64 tile;
    (1000, 384, 1536): several steps per chunk.  g arrives with its largest entry in [2^9, 2^10).  Products of f16
    numbers are exact in fp32, so only the accumulation (rows terms) and the final scale round:
    bound = rows * 2^-24 * max sum |g| |x| + 2^-24 * max|ref|."""
    from isfusion_amd import _lib, swin
    r = _gen(R + N + K)
    g, x = r(R, N), r(R, K)
    gs, sc = _lib.grad_rescale(g.float())
    assert 2.0 ** 9 <= float(gs.abs().max()) < 2.0 ** 10
    xin = x.half() if x16 else x.float().contiguous()
    got = swin.rows_weight_grad_f16(gs, xin, sc[1:])
    g16, x16d = gs.half().double(), xin.half().double()
    inv = float(sc[1])
    ref = (g16.t() @ x16d) * inv
    bound = R * U32 * float((g16.abs().t() @ x16d.abs()).max()) * inv + U32 * float(ref.abs().max())
    e = float((got.double() - ref).abs().max())
    print(f"dW f16 ({R}, {N}, {K}) x16={x16}: err {e:.3e}  bound {bound:.3e}  chunks "
          f"{_lib.load().isf_rows_weight_grad_chunks(R, N, K)}")
    assert got.dtype == torch.float32 and e <= bound, (e, bound)
    assert torch.equal(got, swin.rows_weight_grad_f16(gs, xin, sc[1:]))


# ------------------------------------------------------------------------------------------ 3. attention backward
_ATT = {}


def _attention(case, wide=False):
    key = (case, wide)
    if key not in _ATT:
        t = CM.attention_inputs(case, CM.V_BOUND if wide else None)
        _ATT[key] = (t, CM.attention_yardsticks(case, t, "cuda"))
    return _ATT[key]


def _attention_run(case, t, rescale):
    """-> (dqkv, drel, dtable, pad) in the upstream's own scale"""
    from isfusion_amd import _lib, swin
    B, H, W, heads, shift = CM.ATTENTION[case]
    C = 32 * heads
    qkv, bias, table, index = t["qkv"].to(DEV), t["bias"].to(DEV), t["table"].to(DEV), t["index"].to(DEV)
    rel = table[index.view(-1)].view(49, 49, heads).permute(2, 0, 1).contiguous()
    dout, inv = t["up"].float().to(DEV), None
    back = 1.0
    if rescale:
        dout, sc = _lib.grad_rescale(dout)
        assert 2.0 ** 9 <= float(dout.abs().max()) < 2.0 ** 10
        inv, back = sc[1:], float(sc[1])

    def run():
        return swin.window_attention_backward(qkv, bias, rel, dout, B, H, W, C, heads, 7, shift, 32 ** -0.5,
                                              rel_index=index, table_rows=169, inv_scale=inv)

    first, again = run(), run()
    for a, b in zip(first, again):
        assert a.dtype == torch.float32 and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    dqkv, drel, dtable, pad = first
    return dqkv * back, drel * back, dtable, pad * back


def _attention_check(case, wide, rescale):
    B, H, W, heads, shift = CM.ATTENTION[case]
    C = 32 * heads
    t, (ref, ac) = _attention(case, wide)
    dqkv, drel, dtable, pad = _attention_run(case, t, rescale)
    tag = f"attention {CM.ATTENTION[case]}" + (" |v| <= 32" if wide else "") + (" rescaled" if rescale else " unit")
    CM.rule(f"{tag} dqkv", dqkv, ref[1], ac[1], ROWS)
    CM.rule(f"{tag} dqkv_bias", pad, ref[2], ac[2], PARAMS)
    CM.rule(f"{tag} dtable", dtable, ref[3], ac[3], PARAMS)
    # the gathered-bias gradient folds into the table gradient (fp32 sums of 49 * 49 * heads / 169 terms each)
    fold = torch.zeros(169, heads, dtype=torch.float64, device=DEV).index_add_(
        0, t["index"].to(DEV).view(-1), drel.double().permute(1, 2, 0).reshape(49 * 49, heads))
    assert float((fold - dtable.double()).abs().max()) <= 1e-5 * float(fold.abs().max())
    assert bool((pad[:C] == 0).all())                                    # a padded query has no gradient
    if H % 7 or W % 7:
        assert float(pad[C:].abs().max()) > 1e-2                         # padded keys and values take part
    else:
        assert bool((pad == 0).all())


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("case", range(len(CM.ATTENTION)))
def test_window_attention_backward_f16(case, rescale):
    from isfusion_amd import swin
    B, H, W, heads, shift = CM.ATTENTION[case]
    t, (ref, ac) = _attention(case)
    if not rescale:
        # the forward the backward recomputes is the f16 forward kernel's
        rel = t["table"][t["index"].view(-1)].view(49, 49, heads).permute(2, 0, 1).contiguous().to(DEV)
        out = swin.window_attention(t["qkv"].to(DEV), t["bias"].to(DEV), rel, B, H, W, 32 * heads, heads, 7, shift,
                                    32 ** -0.5)
        CM.rule(f"attention {CM.ATTENTION[case]} out", out, ref[0], ac[0], ROWS)
    _attention_check(case, False, rescale)


def test_window_attention_backward_f16_at_the_stated_value_range():
    """v entries up to the header's bound (32) and dout's largest entry in [2^9, 2^10): finite, within the rule"""
    t, _ = _attention(CM.RANGE_CASE, True)
    C = 32 * CM.ATTENTION[CM.RANGE_CASE][3]
    assert float(t["qkv"][:, 2 * C:].abs().max()) == CM.V_BOUND
    _attention_check(CM.RANGE_CASE, True, True)


# -------------------------------------------------------------------------------------------------- 4. one SwinBlock
def _autocast(dtype):
    return torch.autocast("cuda", dtype=torch.float16, enabled=dtype == torch.float32)


def _block_torch(sd, x, up, hw, shift, keep, dtype):
    p = CT.leaf_params(sd, dtype, DEV)
    x = x.detach().clone().to(dtype).requires_grad_(True)
    with _autocast(dtype):
        out = CT.swin_block_train(p, "", x, hw, 3, 7, shift, keep.to(dtype), keep.to(dtype))
    (out.to(dtype) * up.to(dtype).view_as(out)).sum().backward()
    return out.detach(), x.grad, {k: v.grad for k, v in p.items() if v.requires_grad}


def _block_run(blk, x, up, B, H, W, keep):
    from isfusion_amd import _lib
    from isfusion_amd.swin import PackedLinearF16
    p, pb = blk.pack(PackedLinearF16), blk.pack_backward(PackedLinearF16)
    tape = []
    out = blk.run(p, x, B, H, W, (keep, keep), tape)
    assert tape[0]["qkv"].dtype == tape[0]["att"].dtype == torch.float16       # what the forward keeps: f16 rows
    assert tape[0]["x"].dtype == tape[0]["y"].dtype == torch.float32
    gs, sc = _lib.grad_rescale(up)
    grads = {}
    dx = blk.run_backward(p, pb, tape[0], gs, B, H, W, sc[1:], grads) * sc[1]
    names = {q: n for n, q in blk.named_parameters()}
    return out, dx, {names[q]: v for q, v in grads.items()}


@pytest.mark.parametrize("shift", [0, 3])
def test_swin_block_mixed(shift):
    from isfusion_amd.swin import SwinBlock
    B, H, W, C = 3, 9, 10, 96
    blk = SwinBlock(96, 3, 384, 7, shift=shift > 0)
    blk.load_state_dict(CC.seeded_module_state(blk, 900 + int(shift > 0)))
    blk = blk.to(DEV)
    r = _gen(50 + shift)
    x, up = r(B, H * W, C), r(B * H * W, C) / (B * H * W * C) ** 0.5
    s = torch.tensor([1 / 0.8, 0.0, 1 / 0.8], dtype=torch.float64, device=DEV)
    sd = blk.state_dict()
    ref = _block_torch(sd, x, up, (H, W), shift, s, torch.float64)
    ac = _block_torch(sd, x, up, (H, W), shift, s, torch.float32)
    sf = s.float().contiguous()
    xf, upf = x.float().view(-1, C).contiguous(), up.float().contiguous()
    out, dx, grads = _block_run(blk, xf, upf, B, H, W, sf)
    tag = f"mixed block shift {shift}"
    CM.rule(f"{tag} out", out, ref[0].view(-1, C), ac[0].view(-1, C), ROWS)
    CM.rule(f"{tag} dx", dx, ref[1].view(-1, C), ac[1].view(-1, C), ROWS)
    assert sorted(grads) == sorted(ref[2]) and len(grads) == 13
    for name in sorted(grads):
        assert grads[name].shape == ref[2][name].shape and grads[name].dtype == torch.float32
        CM.rule(f"{tag} grad {name}", grads[name], ref[2][name], ac[2][name], PARAMS)
    mid = slice(H * W, 2 * H * W)                 # the dropped image: only the identity path carries its gradient
    assert torch.equal(dx[mid], upf[mid]) and torch.equal(out[mid], xf[mid])
    again = _block_run(blk, xf, upf, B, H, W, sf)
    assert torch.equal(out, again[0]) and torch.equal(dx, again[1])
    assert all(torch.equal(grads[n], again[2][n]) for n in grads)


# ------------------------------------------------------------------------------------ 5. PatchMerging and PatchEmbed
@pytest.mark.parametrize("H,W", [(9, 11), (8, 10)])
def test_patch_merging_mixed(H, W):
    from isfusion_amd import _lib
    from isfusion_amd.swin import PackedLinearF16, PatchMerging
    B, C = 2, 96
    pm = PatchMerging(C, 2 * C)
    pm.load_state_dict(CC.seeded_module_state(pm, 910))
    pm = pm.to(DEV)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    r = _gen(H * W)
    x, up = r(B, H * W, C), r(B * Ho * Wo, 2 * C) / (B * Ho * Wo * 2 * C) ** 0.5
    res = {}
    for dtype in (torch.float64, torch.float32):
        p = CT.leaf_params(pm.state_dict(), dtype, DEV)
        xx = x.detach().clone().to(dtype).requires_grad_(True)
        with _autocast(dtype):
            out, hw = CC.patch_merging(p, "", xx, (H, W))
        (out.to(dtype).reshape(-1, 2 * C) * up.to(dtype)).sum().backward()
        res[dtype] = (out.detach().reshape(-1, 2 * C), xx.grad.view(-1, C), {k: v.grad for k, v in p.items()})
    p, tape = pm.pack(PackedLinearF16), []
    xf = x.float().view(-1, C).contiguous()
    out, _ = pm.run(p, xf, B, H, W, tape)
    gs, sc = _lib.grad_rescale(up.float())
    grads = {}
    dx = pm.run_backward(p, pm.pack_backward(p, PackedLinearF16), tape[0], gs, B, H, W, sc[1:], grads) * sc[1]
    tag = f"mixed merging {H}x{W}"
    CM.rule(f"{tag} out", out, res[torch.float64][0], res[torch.float32][0], ROWS)
    CM.rule(f"{tag} dx", dx, res[torch.float64][1], res[torch.float32][1], ROWS)
    names = {q: n for n, q in pm.named_parameters()}
    assert sorted(names[q] for q in grads) == ["norm.bias", "norm.weight", "reduction.weight"]
    for q, v in grads.items():
        assert v.shape == q.shape and v.dtype == torch.float32
        CM.rule(f"{tag} grad {names[q]}", v, res[torch.float64][2][names[q]], res[torch.float32][2][names[q]], PARAMS)


def test_patch_embed_mixed():
    from isfusion_amd import _lib
    from isfusion_amd.swin import PackedLinearF16, PatchEmbed
    pe = PatchEmbed(3, 96, 4, 4, dict(type="LN"))
    pe.load_state_dict(CC.seeded_module_state(pe, 920))
    pe = pe.to(DEV)
    img = CC.images(41, 2, 90, 150).to(DEV)
    M = 2 * 23 * 38
    up = _gen(41)(M, 96) / (M * 96) ** 0.5
    res = {}
    for dtype in (torch.float64, torch.float32):
        p = CT.leaf_params({"patch_embed." + k: v for k, v in pe.state_dict().items()}, dtype, DEV)
        with _autocast(dtype):
            out, hw = CC.patch_embed(p, img.to(dtype))
        assert hw == (23, 38)
        (out.to(dtype).reshape(M, 96) * up.to(dtype)).sum().backward()
        res[dtype] = (out.detach().reshape(M, 96), {k[len("patch_embed."):]: v.grad for k, v in p.items()})
    p, tape = pe.pack(PackedLinearF16), []
    out, _ = pe.run(p, img, tape)
    gs, sc = _lib.grad_rescale(up.float())
    grads = {}
    pe.run_backward(tape[0], gs, sc, grads, f16=True)
    CM.rule("mixed patch embed out", out, res[torch.float64][0], res[torch.float32][0], ROWS)
    names = {q: n for n, q in pe.named_parameters()}
    assert sorted(names[q] for q in grads) == ["norm.bias", "norm.weight", "projection.bias", "projection.weight"]
    for q, v in grads.items():
        assert v.shape == q.shape and v.dtype == torch.float32
        CM.rule(f"mixed patch embed grad {names[q]}", v, res[torch.float64][1][names[q]], res[torch.float32][1][names[q]],
                PARAMS)


# ------------------------------------------------------------------------------------------------ 6. whole backbone
def _backbone_hip(bb, img, keep, ups):
    bb.zero_grad(set_to_none=True)
    outs = bb.forward_train(img, drop_keep=keep, backward=True)
    assert all(o.requires_grad and o.dtype == torch.float32 for o in outs)
    sum((o * u.float()).sum() for o, u in zip(outs, ups)).backward()
    return [o.detach() for o in outs], {n: q.grad.detach().clone() for n, q in bb.named_parameters()}


@pytest.mark.parametrize("size", CT.TRAIN_SIZES)
def test_backbone_mixed_meets_the_rule(size):
    sd, img, keep = CM.backbone_inputs(size)
    img, keep = img.to(DEV), keep.to(DEV)
    bb = G._backbone().train().set_precision("mixed")
    plain = bb.forward_train(img, drop_keep=keep)
    assert all(not t.requires_grad and t.dtype == torch.float32 for t in plain)
    ups = [u.to(DEV) for u in CM.upstreams([tuple(t.shape) for t in plain])]
    outs, grads = _backbone_hip(bb, img, keep, ups)
    for a, b in zip(outs, plain):
        assert torch.equal(a, b)                          # the same launches with and without the backward
    o64, g64 = CM.backbone_yardstick(sd, img, keep, ups, torch.float64, "cuda")
    oac, gac = CM.backbone_yardstick(sd, img, keep, ups, torch.float32, "cuda")
    for i, (a, b, c) in enumerate(zip(outs, o64, oac)):
        CM.rule(f"mixed backbone {size} map {i}", a, b, c, ROWS)
    assert sorted(grads) == sorted(g64)
    for name in sorted(grads):
        g = grads[name]
        assert g.dtype == torch.float32 and g.shape == g64[name].shape, name
        CM.rule(f"mixed backbone {size} grad {name}", g, g64[name], gac[name], PARAMS)
    again = _backbone_hip(bb, img, keep, ups)[1]
    assert all(torch.equal(grads[n], again[n]) for n in grads)          # a second backward, bit for bit


def test_backbone_mixed_does_not_leak_into_the_other_modes():
    size = CT.TRAIN_SIZES[0]
    sd, img, keep = CM.backbone_inputs(size)
    img, keep = img.to(DEV), keep.to(DEV)
    bb = G._backbone().train()
    ups = [u.to(DEV) for u in CM.upstreams([tuple(t.shape) for t in bb.forward_train(img, drop_keep=keep)])]
    bb.set_precision("mixed")
    mixed = _backbone_hip(bb, img, keep, ups)
    # eval(): the f16 mode's forward, bit for bit, on the same packed weights
    bb.eval()
    ev = bb(img)
    from isfusion_amd.derived import store as derived_store
    store = derived_store(bb, DEV)
    assert "f16" in store and "f16_backward" in store and "mixed" not in store
    bb.set_precision("f16")
    for a, b in zip(ev, bb(img)):
        assert torch.equal(a, b)
    # "f32" -> "mixed" -> "f32" == never left "f32"
    bb.train().set_precision("f32")
    back = _backbone_hip(bb, img, keep, ups)
    fresh = _backbone_hip(G._backbone().train(), img, keep, ups)
    assert all(torch.equal(a, b) for a, b in zip(back[0], fresh[0]))
    assert all(torch.equal(back[1][n], fresh[1][n]) for n in fresh[1])
    assert not torch.equal(mixed[0][0], fresh[0][0])                    # and really another arithmetic
    # new weights while in mixed mode: the forward and the transposed packs are both derived again
    bb.set_precision("mixed")
    bb.load_state_dict(CC.seeded_module_state(bb, G.BACKBONE_SEED + 1), strict=True)
    other = G._backbone()
    other.load_state_dict(CC.seeded_module_state(other, G.BACKBONE_SEED + 1))
    want = _backbone_hip(other.train().set_precision("mixed"), img, keep, ups)
    got = _backbone_hip(bb, img, keep, ups)
    assert all(torch.equal(a, b) for a, b in zip(got[0], want[0])) and not torch.equal(got[0][0], mixed[0][0])
    assert all(torch.equal(got[1][n], want[1][n]) for n in want[1])
    # changing the mode between the forward and its backward is refused
    outs = bb.forward_train(img, drop_keep=keep, backward=True)
    bb.set_precision("f32")
    with pytest.raises(RuntimeError, match="precision"):
        sum((o * u.float()).sum() for o, u in zip(outs, ups)).backward()


# ------------------------------------------------------------------------------------------------------ 7. detector
def test_detector_camera_precision_mixed():
    with G._rng_restored():
        try:
            _detector_mixed()
        finally:
            G._DET.clear()


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _detector_mixed():
    import ast
    import os
    from isfusion_amd import optim
    from test_gpu_swin_backward import _on_stride16_path
    d = G._detector()
    det = G._fresh(d)
    det.detach = False
    det.camera_backward = True
    try:
        ld32, neck32, _, _ = G._detector_step(d)
        ld32 = {k: v.detach().clone() for k, v in ld32.items()}
        det.camera_precision = "mixed"
        assert det.img_backbone.precision == "mixed"
        ld, neck, _, det = G._detector_step(d)
        assert all(bool(torch.isfinite(v).all()) for v in ld.values())
        for name, q in det.named_parameters():
            if name.startswith("img_backbone."):
                if _on_stride16_path(name):
                    assert q.grad is not None and q.grad.dtype == torch.float32, name
                    assert bool(torch.isfinite(q.grad).all()) and float(q.grad.abs().max()) > 0, name
                else:
                    assert q.grad is None, name
        # against the f32 mode on the same inputs: recorded, not bounded (the points path makes a discrete choice that is
        # not reproducible run to run)
        print("detector mixed vs f32: largest relative loss difference "
              f"{max(_rel(ld[k], ld32[k]) for k in ld if k != 'matched_ious'):.3e}, largest relative img_neck gradient "
              f"difference {max(_rel(neck[k], neck32[k]) for k in neck):.3e}")
        with open(os.path.join(G.HERE, "golden", "isfusion_0075voxel_train.txt")) as f:
            cfg = ast.literal_eval(f.read())["optimizer"]
        before = det.img_backbone.stages[2].blocks[1].ffn.layers[1].weight.detach().clone()
        optim.build_optimizer(det, cfg).step()
        after = det.img_backbone.stages[2].blocks[1].ffn.layers[1].weight
        assert bool(torch.isfinite(after).all()) and not torch.equal(after, before)
        # the shipped setting: the maps are detached and the backbone gets no gradient
        det = G._fresh(d)
        det.detach = True
        feats = det.extract_img_feat(d["img"].clone(), [dict(m) for m in d["metas"]])
        feats[1].sum().backward()
        assert all(q.grad is None for q in det.img_backbone.parameters())
        assert any(q.grad is not None for q in det.img_neck.parameters())
    finally:
        det.detach = True
        det.camera_precision = "f32"
        if "camera_backward" in det.__dict__:
            del det.camera_backward
