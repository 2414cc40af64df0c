"""GPU tests of the camera backbone's backward (csrc/isf_swin_train.hip, SwinTransformer.forward_train(backward=True),
GeneralizedLSSFPN.forward_train(input_grads=True), ISFusionDetector.camera_backward): every new kernel, one block, the
merging / embedding layers, the whole backbone, the neck's input gradients, the detector and one optimizer step, against
float64 autograd over the restatements of tests/camera_common.py / tests/camera_train_common.py.

Tolerance, the camera branch's convention (tests/test_gpu_camera_train.py::_within): err(HIP vs float64) <= 2 x
err(float32 stock torch, same inputs, same GPU, vs float64) + floor, with floor = 2e-6 x max|ref| for single kernels and
1e-4 for whole modules, whose upstream gradients are scaled by 1 / sqrt(elements) so parameter gradients are of order 1."""
import os

import pytest
import torch
import torch.nn.functional as F

import camera_common as CC
import camera_train_common as CT
import test_gpu_camera_train as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_within, _gen = G._within, G._gen
WS = 7


# ------------------------------------------------------------------------------------- 1. window-attention backward
def _attention_core(qkv, bias, table, index, B, H, W, heads, shift):
    """ShiftWindowMSA between the qkv Linear and proj (camera_common.shift_window_msa), from qkv rows [B*H*W, 3C]: the
    pad to multiples of 7 comes after the Linear's input was padded with zeros, so a padded cell's q / k / v are `bias`"""
    C3 = qkv.shape[1]
    C = C3 // 3
    hd = C // heads
    x = qkv.view(B, H, W, C3)
    pr, pb = (WS - W % WS) % WS, (WS - H % WS) % WS
    Hp, Wp = H + pb, W + pr
    inside = torch.zeros((1, Hp, Wp, 1), dtype=torch.bool, device=qkv.device)
    inside[:, :H, :W] = True
    x = torch.where(inside, F.pad(x, (0, 0, 0, pr, 0, pb)), bias.view(1, 1, 1, C3).expand(B, Hp, Wp, C3))
    mask = None
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
        lab = torch.zeros((1, Hp, Wp, 1), dtype=x.dtype, device=x.device)
        cnt = 0
        for hs in (slice(0, -WS), slice(-WS, -shift), slice(-shift, None)):
            for wsl in (slice(0, -WS), slice(-WS, -shift), slice(-shift, None)):
                lab[:, hs, wsl, :] = cnt
                cnt += 1
        mw = CC._windows(lab, WS).squeeze(-1)
        d = mw.unsqueeze(1) - mw.unsqueeze(2)
        mask = torch.where(d != 0, torch.full_like(d, -100.0), torch.zeros_like(d))
    win = CC._windows(x, WS)
    nW_, N, _ = win.shape
    w = win.reshape(nW_, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = w[0] * (hd ** -0.5), w[1], w[2]
    rel = table[index.view(-1)].view(N, N, heads).permute(2, 0, 1)
    attn = q @ k.transpose(-2, -1) + rel.unsqueeze(0)
    if mask is not None:
        nw = mask.shape[0]
        attn = (attn.view(-1, nw, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    o = (attn.softmax(-1) @ v).transpose(1, 2).reshape(nW_, N, C)
    x = CC._unwindows(o, B, Hp, Wp, WS)
    if shift > 0:
        x = torch.roll(x, shifts=(shift, shift), dims=(1, 2))
    return x[:, :H, :W, :].reshape(B * H * W, C)


ATTENTION = [(1, 7, 7, 3, 0),       # one window, no padding
             (2, 9, 10, 3, 0),      # 2 x 2 windows, padding on both axes
             (2, 9, 10, 3, 3),      # ... and every shift region
             (2, 14, 21, 6, 3),     # no padding, shift only, C = 192
             (1, 3, 5, 3, 3)]       # grid smaller than a window
_ATT = {}


def _attention_case(case):
    """inputs and the float64 / float32 gradients for a unit-scale upstream, computed once (the backward is linear in
    the upstream, so the 2^k cases scale these)"""
    if case in _ATT:
        return _ATT[case]
    from isfusion_amd.swin import WindowMSA
    B, H, W, heads, shift = ATTENTION[case]
    C = 32 * heads
    r = _gen(4000 + case)
    index = WindowMSA(C, heads, (WS, WS)).relative_position_index.to(DEV)
    t = dict(qkv=r(B * H * W, 3 * C), bias=r(3 * C, s=0.3), table=r(169, heads, s=0.5), up=r(B * H * W, C), index=index)
    for dtype in (torch.float64, torch.float32):
        leaves = [t[k].detach().clone().to(dtype).requires_grad_(True) for k in ("qkv", "bias", "table")]
        out = _attention_core(*leaves, index, B, H, W, heads, shift)
        t[dtype] = torch.autograd.grad(out, leaves, t["up"].to(dtype))
    _ATT[case] = t
    return t


@pytest.mark.parametrize("log2_scale", [0, -20, 10])
@pytest.mark.parametrize("case", range(len(ATTENTION)))
def test_window_attention_backward(case, log2_scale):
    from isfusion_amd import swin
    B, H, W, heads, shift = ATTENTION[case]
    C = 32 * heads
    t = _attention_case(case)
    s = 2.0 ** log2_scale
    qkv, bias, table = (t[k].float().contiguous() for k in ("qkv", "bias", "table"))
    rel = table[t["index"].view(-1)].view(49, 49, heads).permute(2, 0, 1).contiguous()
    # the forward the backward recomputes: the kernel's own output equals the restatement's
    out = swin.window_attention(qkv, bias, rel, B, H, W, C, heads, WS, shift, 32 ** -0.5)
    ref_out = _attention_core(t["qkv"], t["bias"], t["table"], t["index"], B, H, W, heads, shift)
    assert float((out.double() - ref_out).abs().max()) < 1e-5 * float(ref_out.abs().max())
    dout = (t["up"] * s).float().contiguous()

    def run():
        return swin.window_attention_backward(qkv, bias, rel, dout, B, H, W, C, heads, WS, shift, 32 ** -0.5,
                                              rel_index=t["index"], table_rows=169)

    dqkv, drel, dtable, pad = run()
    tag = f"attention {ATTENTION[case]} 2^{log2_scale}"
    names = ("dqkv", "dqkv_bias", "dtable")
    for name, got, ref, f32 in zip(names, (dqkv, pad, dtable), (t[torch.float64][i] for i in (0, 1, 2)),
                                   (t[torch.float32][i] for i in (0, 1, 2))):
        _within(f"{tag} {name}", got, ref * s, f32 * s, floor_rel=2e-6)
    # the gathered-bias gradient folds into the table gradient
    fold = torch.zeros(169, heads, dtype=torch.float64, device=DEV).index_add_(
        0, t["index"].view(-1), drel.double().permute(1, 2, 0).reshape(49 * 49, heads))
    assert float((fold - dtable.double()).abs().max()) <= 1e-5 * float(fold.abs().max())
    padded = H % WS != 0 or W % WS != 0
    ref_pad = t[torch.float64][1]
    assert bool((ref_pad[:C] == 0).all()) and bool((pad[:C] == 0).all())     # a padded query has no gradient
    if padded:
        # the share the test is here for: padded keys and values take part, their dK / dV are the bias's
        assert float(ref_pad[C:].abs().max()) > 1e-2 and float(pad[C:].abs().max()) > 1e-2 * s
    else:
        assert bool((ref_pad == 0).all()) and bool((pad == 0).all())
    for a, b in zip((dqkv, drel, dtable, pad), run()):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ 2. LayerNorm backward
def _ln_torch(x, gamma, beta, dy, res):
    x = x.detach().clone().requires_grad_(True)
    gamma, beta = gamma.detach().clone().requires_grad_(True), beta.detach().clone().requires_grad_(True)
    y = F.layer_norm(x, (x.shape[-1],), gamma, beta, 1e-5)
    dx, dg, db = torch.autograd.grad(y, (x, gamma, beta), dy)
    return (dx + res if res is not None else dx), dg, db


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("M,K,B", [(105, 96, 3), (130, 384, 2), (270, 768, 2)])
def test_layernorm_backward(M, K, B, residual):
    """105 / 130 / 270 rows: ragged last chunks, several chunks, a wave with no row; 105 = 3 x 35: an odd hw for the NCHW
    incoming gradient"""
    from isfusion_amd import _lib, swin
    assert _lib.load().isf_swin_layernorm_backward_parts(M) > 4
    r = _gen(M + K)
    x, gamma, beta, dy = r(M, K), 1.0 + r(K, s=0.1), r(K, s=0.1), r(M, K)
    res = r(M, K) if residual else None
    ref = _ln_torch(x, gamma, beta, dy, res)
    f32 = _ln_torch(x.float(), gamma.float(), beta.float(), dy.float(), None if res is None else res.float())
    xf = x.float().contiguous()
    st = swin.row_stats(swin._a(_lib.SWIN_A_ROWS, xf, ldx=K), M, K, 1e-5)
    a = swin._a(_lib.SWIN_A_ROWS, xf, ldx=K, stats=st, ln=(gamma.float(), beta.float()))
    resf = None if res is None else res.float().contiguous()
    layouts = [("rows", dy.float().contiguous(), 0)]
    if M == 105:
        hw = M // B
        layouts.append(("nchw", dy.float().view(B, hw, K).permute(0, 2, 1).contiguous(), hw))
    for name, dyl, hw in layouts:
        got = swin.layernorm_backward(a, M, K, dyl, dy_hw=hw, residual=resf)
        for what, g_, r_, f_ in zip(("dx", "dgamma", "dbeta"), got, ref, f32):
            _within(f"layernorm backward {name} ({M}, {K}) residual={residual} {what}", g_, r_, f_, floor_rel=2e-6)
        for p, q in zip(got, swin.layernorm_backward(a, M, K, dyl, dy_hw=hw, residual=resf)):
            assert torch.equal(p, q)
    # the two scalar factors: dy_scale on the way in, inv_scale on the parameter gradients
    two, half = torch.tensor([2.0], device=DEV), torch.tensor([0.5], device=DEV)
    plain = swin.layernorm_backward(a, M, K, layouts[0][1])
    scaled = swin.layernorm_backward(a, M, K, layouts[0][1], dy_scale=two, inv_scale=half)
    assert torch.equal(scaled[0], plain[0] * 2) and torch.equal(scaled[1], plain[1]) and torch.equal(scaled[2], plain[2])


# ------------------------------------------------------------------------- small kernels: GELU', column sums, row scale
def test_gelu_backward_column_sums_and_row_scale():
    from isfusion_amd import swin
    r = _gen(77)
    M, N = 270, 384
    z, g = r(M, N, s=2.0), r(M, N)
    z64 = z.clone().requires_grad_(True)
    h64 = F.gelu(z64)
    dz64, = torch.autograd.grad(h64, z64, g)
    z32 = z.float().requires_grad_(True)
    h32 = F.gelu(z32)
    dz32, = torch.autograd.grad(h32, z32, g.float())
    h, dz = z.float().contiguous(), g.float().contiguous()
    swin.gelu_backward(h, dz)
    _within("gelu backward h", h, h64.detach(), h32.detach(), floor_rel=2e-6)
    _within("gelu backward dz", dz, dz64, dz32, floor_rel=2e-6)
    gf = g.float().contiguous()
    extra = r(N).float()
    inv = torch.tensor([0.25], device=DEV)
    got = swin.column_sums(gf, extra=extra, inv_scale=inv)
    _within("column sums", got, (g.sum(0) + extra.double()) * 0.25, (gf.sum(0) + extra) * 0.25, floor_rel=2e-6)
    assert torch.equal(got, swin.column_sums(gf, extra=extra, inv_scale=inv))
    s = torch.tensor([1.25, 0.0, 1.25], device=DEV)
    rows = swin.scale_rows(gf, s)
    assert torch.equal(rows, gf * s.repeat_interleave(M // 3)[:, None]) and bool((rows[90:180] == 0).all())
    assert swin.scale_rows(gf, None) is gf


# -------------------------------------------------------------------------------------------------- 3. one SwinBlock
def _block(shift):
    from isfusion_amd.swin import SwinBlock
    blk = SwinBlock(96, 3, 384, 7, shift=shift)
    blk.load_state_dict(CC.seeded_module_state(blk, 900 + int(shift)))
    return blk.to(DEV)


def _block_run(blk, x, up, B, H, W, keep):
    """forward + backward of one block on token rows x [B*H*W, C] -> (output rows, dx, {state-dict name: gradient})"""
    from isfusion_amd import _lib
    p, pb = blk.pack(), blk.pack_backward()
    tape = []
    out = blk.run(p, x, B, H, W, keep, tape)
    gs, sc = _lib.grad_rescale(up)
    grads = {}
    dx = blk.run_backward(p, pb, tape[0], gs, B, H, W, sc[1:], grads) * sc[1]
    names = {q: n for n, q in blk.named_parameters()}
    return out, dx, {names[q]: v for q, v in grads.items()}


def _block_torch(sd, x, up, hw, shift, keep, dtype):
    p = CT.leaf_params(sd, dtype, DEV)
    x = x.detach().clone().to(dtype).requires_grad_(True)
    out = CT.swin_block_train(p, "", x, hw, 3, 7, shift, keep[0].to(dtype), keep[1].to(dtype))
    (out * up.to(dtype).view_as(out)).sum().backward()
    return out.detach(), x.grad, {k: v.grad for k, v in p.items() if v.requires_grad}


@pytest.mark.parametrize("shift", [0, 3])
def test_swin_block_forward_backward(shift):
    B, H, W, C = 3, 9, 10, 96
    blk = _block(shift > 0)
    assert blk.attn.shift_size == shift
    r = _gen(50 + shift)
    x, up = r(B, H * W, C), r(B * H * W, C) / (B * H * W * C) ** 0.5
    s = torch.tensor([1 / 0.8, 0.0, 1 / 0.8], dtype=torch.float64, device=DEV)
    sd = blk.state_dict()
    ref = _block_torch(sd, x, up, (H, W), shift, (s, s), torch.float64)
    f32 = _block_torch(sd, x, up, (H, W), shift, (s, s), torch.float32)
    sf = s.float().contiguous()
    xf, upf = x.float().view(-1, C).contiguous(), up.float().contiguous()
    out, dx, grads = _block_run(blk, xf, upf, B, H, W, (sf, sf))
    tag = f"block shift {shift}"
    _within(f"{tag} out", out, ref[0].view(-1, C), f32[0].view(-1, C), floor_abs=1e-4)
    _within(f"{tag} dx", dx, ref[1].view(-1, C), f32[1].view(-1, C), floor_abs=1e-4)
    assert sorted(grads) == sorted(ref[2]) and len(grads) == 13       # twelve of the issue's + the bias table
    for name in sorted(grads):
        assert grads[name].shape == ref[2][name].shape and grads[name].dtype == torch.float32
        _within(f"{tag} grad {name}", grads[name], ref[2][name], f32[2][name], floor_abs=1e-4)
    # the dropped image: only the identity path carries its gradient, and it adds nothing to a branch parameter
    mid = slice(H * W, 2 * H * W)
    assert torch.equal(dx[mid], upf[mid])
    two = [0, 2]
    x2, up2 = x[two], up.view(B, H * W, C)[two].reshape(-1, C)
    ref2 = _block_torch(sd, x2, up2, (H, W), shift, (s[two], s[two]), torch.float64)
    f322 = _block_torch(sd, x2, up2, (H, W), shift, (s[two], s[two]), torch.float32)
    for name in sorted(grads):
        if name.startswith(("attn.", "ffn.")):
            _within(f"{tag} grad {name} vs the two kept images alone", grads[name], ref2[2][name], f322[2][name],
                    floor_abs=1e-4)
    again = _block_run(blk, xf, upf, B, H, W, (sf, sf))
    assert torch.equal(dx, again[1]) and all(torch.equal(grads[n], again[2][n]) for n in grads)


# ------------------------------------------------------------------------------------ 4. PatchMerging and PatchEmbed
@pytest.mark.parametrize("H,W", [(9, 11), (8, 10)])
def test_patch_merging_backward(H, W):
    from isfusion_amd import _lib
    from isfusion_amd.swin import PatchMerging
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
        out, hw = CC.patch_merging(p, "", xx, (H, W))
        assert hw == (Ho, Wo)
        (out.reshape(-1, 2 * C) * up.to(dtype)).sum().backward()
        res[dtype] = (xx.grad.view(-1, C), {k: v.grad for k, v in p.items()})
    p, tape = pm.pack(), []
    xf = x.float().view(-1, C).contiguous()
    pm.run(p, xf, B, H, W, tape)
    gs, sc = _lib.grad_rescale(up.float())
    grads = {}
    dx = pm.run_backward(p, pm.pack_backward(p), tape[0], gs, B, H, W, sc[1:], grads) * sc[1]
    tag = f"merging {H}x{W}"
    _within(f"{tag} dx", dx, res[torch.float64][0], res[torch.float32][0], floor_abs=1e-4)
    names = {q: n for n, q in pm.named_parameters()}
    assert sorted(names[q] for q in grads) == ["norm.bias", "norm.weight", "reduction.weight"]
    for q, v in grads.items():
        assert v.shape == q.shape
        _within(f"{tag} grad {names[q]}", v, res[torch.float64][1][names[q]], res[torch.float32][1][names[q]],
                floor_abs=1e-4)


def test_patch_embed_backward():
    from isfusion_amd import _lib
    from isfusion_amd.swin import PatchEmbed
    pe = PatchEmbed(3, 96, 4, 4, dict(type="LN"))
    pe.load_state_dict(CC.seeded_module_state(pe, 920))
    pe = pe.to(DEV)
    img = CC.images(41, 2, 90, 150).to(DEV)
    M = 2 * 23 * 38
    up = _gen(41)(M, 96) / (M * 96) ** 0.5
    res = {}
    for dtype in (torch.float64, torch.float32):
        p = CT.leaf_params({"patch_embed." + k: v for k, v in pe.state_dict().items()}, dtype, DEV)
        out, hw = CC.patch_embed(p, img.to(dtype))
        assert hw == (23, 38)
        (out.reshape(M, 96) * up.to(dtype)).sum().backward()
        res[dtype] = {k[len("patch_embed."):]: v.grad for k, v in p.items()}
    p, tape = pe.pack(), []
    pe.run(p, img, tape)
    gs, sc = _lib.grad_rescale(up.float())
    grads = {}
    pe.run_backward(tape[0], gs, sc, grads)
    names = {q: n for n, q in pe.named_parameters()}
    assert sorted(names[q] for q in grads) == ["norm.bias", "norm.weight", "projection.bias", "projection.weight"]
    for q, v in grads.items():
        assert v.shape == q.shape
        _within(f"patch embed grad {names[q]}", v, res[torch.float64][names[q]], res[torch.float32][names[q]],
                floor_abs=1e-4)


# ------------------------------------------------------------------------------------------------ 5. whole backbone
def _backbone_torch(sd, img, keep, ups, dtype):
    p = CT.leaf_params(sd, dtype, DEV)
    outs = CT.swin_forward_train(p, img.to(dtype), keep)
    sum((o * u.to(dtype)).sum() for o, u in zip(outs, ups) if u is not None).backward()
    return [o.detach() for o in outs], p


def _backbone_hip(bb, img, keep, ups):
    bb.zero_grad(set_to_none=True)
    outs = bb.forward_train(img, drop_keep=keep, backward=True)
    assert all(o.requires_grad for o in outs)
    sum((o * u.float()).sum() for o, u in zip(outs, ups) if u is not None).backward()
    return outs, {n: (None if q.grad is None else q.grad.detach().clone()) for n, q in bb.named_parameters()}


def _upstreams(shapes, seed):
    return [CT.upstream(seed + i, s).to(DEV) / float(torch.tensor(s).prod()) ** 0.5 for i, s in enumerate(shapes)]


@pytest.mark.parametrize("size", CT.TRAIN_SIZES)
def test_backbone_backward_equals_float64(size):
    n, h, w = size
    bb = G._backbone().train()
    img = CC.images(31, n, h, w).to(DEV)
    keep = CT.fixed_drop_keep(32, n).to(DEV)
    plain = bb.forward_train(img, drop_keep=keep)
    ups = _upstreams([tuple(t.shape) for t in plain], 700)
    outs, grads = _backbone_hip(bb, img, keep, ups)
    for a, b in zip(outs, plain):
        assert torch.equal(a.detach(), b) and not b.requires_grad
    sd = bb.state_dict()
    o64, p64 = _backbone_torch(sd, img, keep, ups, torch.float64)
    o32, p32 = _backbone_torch(sd, img, keep, ups, torch.float32)
    for i, (a, b, c) in enumerate(zip(outs, o64, o32)):
        _within(f"backbone {size} map {i}", a.detach(), b, c, floor_abs=1e-4)
    assert len(grads) == len(list(bb.parameters())) and img.grad is None
    for name, g in grads.items():
        assert g is not None and g.dtype == torch.float32 and g.shape == p64[name].shape, name
        _within(f"backbone {size} grad {name}", g, p64[name].grad, p32[name].grad, floor_abs=1e-4)


def test_backbone_backward_partial_upstream_determinism_and_accumulation():
    import isfusion_amd
    n, h, w = CT.TRAIN_SIZES[0]
    bb = G._backbone().train()
    img = CC.images(31, n, h, w).to(DEV)
    keep = CT.fixed_drop_keep(32, n).to(DEV)
    shapes = [tuple(t.shape) for t in bb.forward_train(img, drop_keep=keep)]
    ups = _upstreams(shapes, 700)
    ups[0] = None                                     # nothing arrives at the first map
    outs, grads = _backbone_hip(bb, img, keep, ups)
    sd = bb.state_dict()
    o64, p64 = _backbone_torch(sd, img, keep, ups, torch.float64)
    o32, p32 = _backbone_torch(sd, img, keep, ups, torch.float32)
    first = f"norm{CC.BACKBONE['out_indices'][0]}."
    for name, g in grads.items():
        if name.startswith(first):
            assert g is None and p64[name].grad is None, name
            continue
        _within(f"backbone partial upstream grad {name}", g, p64[name].grad, p32[name].grad, floor_abs=1e-4)
    for mode in (False, True):
        with isfusion_amd.deterministic(mode):
            a = _backbone_hip(bb, img, keep, ups)[1]
            b = _backbone_hip(bb, img, keep, ups)[1]
        for name in a:
            assert (a[name] is None and b[name] is None) or torch.equal(a[name], b[name]), (mode, name)
            assert (a[name] is None and grads[name] is None) or torch.equal(a[name], grads[name]), (mode, name)
    # a second backward without zero_grad accumulates, as autograd does
    outs = bb.forward_train(img, drop_keep=keep, backward=True)
    sum((o * u.float()).sum() for o, u in zip(outs, ups) if u is not None).backward()
    q = bb.stages[2].blocks[1].ffn.layers[1].weight
    assert torch.equal(q.grad, 2 * grads["stages.2.blocks.1.ffn.layers.1.weight"])
    # the refusals of today's forward_train hold with the switch on
    bb.set_precision("f16")
    with pytest.raises(NotImplementedError):
        bb.forward_train(img, drop_keep=keep, backward=True)
    bb.set_precision("f32")


# -------------------------------------------------------------------------------------------- 6. neck input gradients
@pytest.mark.parametrize("both", [True, False])
def test_neck_input_gradients(both):
    from isfusion_amd.generalized_lss import GeneralizedLSSFPN
    case = G._neck_case()
    ups = case["ups"]

    def neck():
        nk = GeneralizedLSSFPN(**CC.NECK)
        nk.load_state_dict(case["sd"])
        return nk.to(DEV).train()

    def loss(outs, dtype):
        return (outs[1] * ups[1].to(dtype)).sum() + ((outs[0] * ups[0].to(dtype)).sum() if both else 0.0)

    refs = {}
    for dtype in (torch.float64, torch.float32):
        p = CT.leaf_params(case["sd"], dtype, DEV)
        feats = [f.detach().clone().to(dtype).requires_grad_(True) for f in case["feats"]]
        loss(CT.neck_forward_train(p, feats), dtype).backward()
        refs[dtype] = [f.grad for f in feats]
    nk = neck()
    feats = [f.detach().float().requires_grad_(True) for f in case["feats"]]
    loss(nk.forward_train(feats, input_grads=True), torch.float32).backward()
    for i, f in enumerate(feats):
        if i == 0 and not both:
            assert f.grad is None and refs[torch.float64][0] is None
            continue
        assert f.grad.shape == f.shape and f.grad.dtype == torch.float32
        _within(f"neck both={both} input gradient {i}", f.grad, refs[torch.float64][i], refs[torch.float32][i],
                floor_abs=1e-4)
    plain = neck()
    loss(plain.forward_train([f.float() for f in case["feats"]]), torch.float32).backward()
    for (name, a), (_, b) in zip(nk.named_parameters(), plain.named_parameters()):
        assert (a.grad is None and b.grad is None) or torch.equal(a.grad, b.grad), name
    with pytest.raises(NotImplementedError, match="backward"):
        plain.forward_train(feats)


# ------------------------------------------------------------------------------------------ 7. detector, 8. optimizer
def _camera_grads(det):
    return {n: q.grad.detach().clone() for n, q in det.named_parameters()
            if n.startswith(("img_backbone.", "img_neck.")) and q.grad is not None}


def _on_stride16_path(name):
    """img_backbone parameters between the image and the stride-16 map's inputs: everything but the norm of the first
    output map (only the neck's stride-16 output reaches Point-to-Grid, and it is fed by the last two maps)"""
    return not name.startswith(f"img_backbone.norm{CC.BACKBONE['out_indices'][0]}.")


def test_detector_camera_backward_and_optimizer_step():
    with G._rng_restored():
        try:
            _detector_camera_backward()
        finally:
            G._DET.clear()


def _detector_camera_backward():
    import ast
    from isfusion_amd import optim
    d = G._detector()
    det = G._fresh(d)
    assert type(det).camera_backward is False and "camera_backward" not in det.state_dict()
    det.detach = False
    try:
        with pytest.raises(NotImplementedError, match="Swin"):
            det.extract_img_feat(d["img"].clone(), [dict(m) for m in d["metas"]])
        det.camera_backward = True
        ld, _, arrived, det = G._detector_step(d)
        assert set(ld) == {"loss_heatmap", "loss_heatmap_ins", "layer_-1_loss_cls", "layer_-1_loss_bbox", "matched_ious"}
        assert all(bool(torch.isfinite(v).all()) for v in ld.values())
        got = _camera_grads(det)
        for name, q in det.named_parameters():
            if name.startswith("img_backbone."):
                if _on_stride16_path(name):
                    assert q.grad is not None and q.grad.dtype == torch.float32, name
                    assert bool(torch.isfinite(q.grad).all()) and float(q.grad.abs().max()) > 0, name
                else:
                    assert q.grad is None, name
            elif name.startswith(("img_neck.lateral_convs.1.", "img_neck.fpn_convs.1.")):
                assert q.grad is not None and bool(torch.isfinite(q.grad).all()) and float(q.grad.abs().max()) > 0, name
            elif name.startswith("img_neck."):
                assert q.grad is None, name
        # the gradient that arrived at the stride-16 map, pushed by hand through a repeated camera forward
        det = G._fresh(d)
        feats = det.extract_img_feat(d["img"].clone(), [dict(m) for m in d["metas"]])
        assert feats[1].requires_grad
        feats[1].backward(arrived)
        pushed = _camera_grads(det)
        assert sorted(pushed) == sorted(got)
        for name in sorted(got):
            err = float((got[name] - pushed[name]).abs().max()) / float(got[name].abs().max())
            if err > 0:
                print(f"detector {name}: captured gradient pushed by hand vs detector {err:.3e}")
            assert err <= 1e-6, (name, err)
        # 8. one FusedAdamW step of the shipped optimizer: img_backbone moves by the 0.1 x lr group's amount
        with open(os.path.join(G.HERE, "golden", "isfusion_0075voxel_train.txt")) as f:
            cfg = ast.literal_eval(f.read())["optimizer"]
        opt = optim.build_optimizer(det, cfg)
        lrs = {id(g["params"][0]): g["lr"] for g in opt.param_groups}
        before = {n: q.detach().clone() for n, q in det.named_parameters() if n.startswith(("img_backbone.", "img_neck."))}
        opt.step()
        for name, q in det.named_parameters():
            if name not in before:
                continue
            lr = lrs[id(q)]
            assert lr == pytest.approx(cfg["lr"] * (0.1 if name.startswith("img_backbone.") else 1.0)), name
            if q.grad is None:
                assert torch.equal(q, before[name]), name
                continue
            # the first AdamW step moves every entry by lr * (sign(g) / (1 + eps / |g|) + weight_decay * p)
            g, p0 = q.grad.double(), before[name].double()
            want = p0 * (1 - lr * cfg["weight_decay"]) - lr * g / (g.abs() + 1e-8)
            top = float((want - p0).abs().max())
            assert 0 < top <= lr * 1.5, (name, top, lr)
            assert float((q.detach().double() - want).abs().max()) <= 1e-3 * lr + 1e-7 * float(p0.abs().max()), name
    finally:
        det.detach = True
        if "camera_backward" in det.__dict__:
            del det.camera_backward
