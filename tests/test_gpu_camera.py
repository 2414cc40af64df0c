"""GPU tests of the camera branch (isf_swin.hip, swin.py, generalized_lss.py, ISFusionDetector): every kernel against
float64 torch on the Swin-T stage grids of a 384 x 1056 image, backbone + neck against the reference's outputs
(tests/golden/camera_ref.npz) and, at full size, against the float64 restatement (tests/camera_common.py), the
detector against ISFusionPtsPath on the camera features, no host syncs, determinism and a strict state-dict round
trip."""
import ast
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import camera_common as CC
from test_camera import BACKBONE_SEED, NECK_SEED, check_summary

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
# (H, W, C, heads) of the four Swin-T stages at 384 x 1056; every one pads to a multiple of 7
STAGES = [(96, 264, 96, 3), (48, 132, 192, 6), (24, 66, 384, 12), (12, 33, 768, 24)]


def _rel(a, ref):
    return float((a.detach().double() - ref).abs().max()) / (float(ref.abs().max()) + 1e-12)


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return lambda *shape, s=1.0: (torch.randn(*shape, generator=g, dtype=torch.float64) * s).to(DEV)


def _packed(w):
    from isfusion_amd.fusion_ops import PackedLinear
    return PackedLinear(w.float().contiguous())


# ---------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("stage", range(4))
@pytest.mark.parametrize("shift", [0, 3])
def test_window_attention_equals_float64(stage, shift):
    from isfusion_amd import swin
    H, W, C, heads = STAGES[stage]
    r = _gen(10 * stage + shift)
    B = 2
    qkv, bias, table = r(B * H * W, 3 * C), r(3 * C, s=0.5), r(heads, 49, 49, s=0.5)
    got = swin.window_attention(qkv.float(), bias.float(), table.float(), B, H, W, C, heads, 7, shift, 32 ** -0.5)
    # float64: padded cells carry qkv = bias (zero input after norm1), roll, windows, masked softmax, reverse, crop
    Hp, Wp = -(-H // 7) * 7, -(-W // 7) * 7
    grid = bias.expand(B, Hp, Wp, 3 * C).clone()
    grid[:, :H, :W] = qkv.view(B, H, W, 3 * C)
    if shift:
        grid = torch.roll(grid, (-shift, -shift), (1, 2))
    win = CC._windows(grid, 7)                                    # [nW, 49, 3C]
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
    ref = o[:, :H, :W].reshape(B * H * W, C)
    assert _rel(got, ref) < 5e-6, _rel(got, ref)


@pytest.mark.parametrize("stage", range(4))
def test_block_linears_equal_float64(stage):
    """qkv with the norm1 prologue, fc1 with the norm2 prologue + GELU, fc2 (K = 4C) with the residual"""
    from isfusion_amd import _lib, swin
    from isfusion_amd.fusion_ops import ACT_GELU
    H, W, C, _ = STAGES[stage]
    M = H * W
    r = _gen(100 + stage)
    x, g, b = r(M, C, s=3.0) + 0.5, 1 + r(C, s=0.1), r(C, s=0.1)
    w1, b1 = r(3 * C, C, s=C ** -0.5), r(3 * C, s=0.1)
    xf = x.float().contiguous()
    st = swin.row_stats(swin._a(_lib.SWIN_A_ROWS, xf, ldx=C), M, C, 1e-5)
    got = swin.gemm(swin._a(_lib.SWIN_A_ROWS, xf, ldx=C, stats=st, ln=(g.float(), b.float())), M, C, _packed(w1),
                    shift=b1.float())
    ref = F.linear(F.layer_norm(x, (C,), g, b, 1e-5), w1, b1)
    assert _rel(got, ref) < 1e-5
    w2, b2 = r(4 * C, C, s=C ** -0.5), r(4 * C, s=0.1)
    got = swin.gemm(swin._a(_lib.SWIN_A_ROWS, xf, ldx=C, stats=st, ln=(g.float(), b.float())), M, C, _packed(w2),
                    shift=b2.float(), act=ACT_GELU)
    h = F.gelu(F.linear(F.layer_norm(x, (C,), g, b, 1e-5), w2, b2))
    assert _rel(got, h) < 1e-5
    w3, b3, res = r(C, 4 * C, s=(4 * C) ** -0.5), r(C, s=0.1), r(M, C)
    got = swin.gemm(swin._a(_lib.SWIN_A_ROWS, h.float().contiguous(), ldx=4 * C), M, 4 * C, _packed(w3),
                    shift=b3.float(), residual=res.float().contiguous())
    assert _rel(got, F.linear(h, w3, b3) + res) < 1e-5


@pytest.mark.parametrize("grid", [(96, 264, 96), (48, 132, 192), (24, 66, 384), (23, 33, 96), (5, 9, 384)])
def test_patch_merging_equals_float64(grid):
    """Unfold (c*4 + kh*2 + kw, corner padding for odd sizes) -> LayerNorm(4C) -> Linear(4C, 2C)"""
    from isfusion_amd.swin import PatchMerging
    H, W, C = grid
    B = 2
    r = _gen(H + W + C)
    m = PatchMerging(C, 2 * C).to(DEV).eval()
    with torch.no_grad():
        m.norm.weight.copy_(1 + r(4 * C, s=0.1))
        m.norm.bias.copy_(r(4 * C, s=0.1))
        m.reduction.weight.copy_(r(2 * C, 4 * C, s=(4 * C) ** -0.5))
    x = r(B * H * W, C, s=2.0)
    got, (Ho, Wo) = m.run(m.pack(), x.float().contiguous(), B, H, W)
    sd = {"m.norm.weight": m.norm.weight.double(), "m.norm.bias": m.norm.bias.double(),
          "m.reduction.weight": m.reduction.weight.double()}
    ref, hw = CC.patch_merging(sd, "m.", x.view(B, H * W, C), (H, W))
    assert (Ho, Wo) == hw
    assert _rel(got.view(B, Ho * Wo, 2 * C), ref) < 1e-5


@pytest.mark.parametrize("hw", [(384, 1056), (90, 150), (33, 46)])
def test_patch_embed_equals_float64(hw):
    from isfusion_amd.swin import PatchEmbed
    H, W = hw
    r = _gen(H * W)
    m = PatchEmbed(3, 96, 4, 4, dict(type="LN")).to(DEV).eval()
    with torch.no_grad():
        m.projection.weight.copy_(r(96, 3, 4, 4, s=0.15))
        m.projection.bias.copy_(r(96, s=0.1))
        m.norm.weight.copy_(1 + r(96, s=0.1))
        m.norm.bias.copy_(r(96, s=0.1))
    img = r(2, 3, H, W)
    got, ghw = m.run(m.pack(), img.float().contiguous())
    sd = {k: v.double() for k, v in (("patch_embed.projection.weight", m.projection.weight),
                                     ("patch_embed.projection.bias", m.projection.bias),
                                     ("patch_embed.norm.weight", m.norm.weight), ("patch_embed.norm.bias", m.norm.bias))}
    ref, rhw = CC.patch_embed(sd, img)
    assert ghw == rhw
    assert _rel(got.view(ref.shape), ref) < 1e-5


@pytest.mark.parametrize("stage", range(4))
def test_output_layernorm_writes_nchw(stage):
    from isfusion_amd import swin
    H, W, C, _ = STAGES[stage]
    r = _gen(300 + stage)
    x = r(2 * H * W, C, s=4.0) + 1.0
    ln = torch.nn.LayerNorm(C).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(1 + r(C, s=0.1))
        ln.bias.copy_(r(C, s=0.1))
    got = swin.layernorm(x.float(), ln, out_nchw=(2, H, W))
    ref = F.layer_norm(x, (C,), ln.weight.double(), ln.bias.double(), 1e-5).view(2, H, W, C).permute(0, 3, 1, 2)
    assert _rel(got, ref) < 2e-6


@pytest.mark.parametrize("level", [0, 1])
def test_neck_top_down_step_equals_float64(level):
    """interpolate(align_corners) + cat + 1x1 conv + BN + ReLU as one GEMM, then the 3x3 ConvModule (dense_conv) on the
    48 x 132 / 24 x 66 grids"""
    from isfusion_amd.generalized_lss import GeneralizedLSSFPN
    r = _gen(400 + level)
    nk = GeneralizedLSSFPN([192, 384, 768], 256, 3).to(DEV).eval()
    nk.load_state_dict(CC.seeded_module_state(nk, 77))
    feats = [r(2, 192, 48, 132), r(2, 384, 24, 66), r(2, 768, 12, 33)]
    got = nk([f.float() for f in feats])
    ref = CC.neck_forward(CC.cast(nk.state_dict(), torch.float64, DEV), feats)
    assert tuple(got[level].shape) == tuple(ref[level].shape)
    assert _rel(got[level], ref[level]) < 1e-5


# ------------------------------------------------------------------------------------------ backbone + neck
def _camera(dev=DEV):
    from test_camera import _modules
    bb, nk = _modules()
    bb.load_state_dict(CC.seeded_module_state(bb, BACKBONE_SEED))
    nk.load_state_dict(CC.seeded_module_state(nk, NECK_SEED))
    return bb.to(dev).eval(), nk.to(dev).eval()


@pytest.mark.parametrize("case", range(len(CC.GOLDEN_SIZES)))
def test_backbone_and_neck_equal_the_reference(case):
    g = np.load(os.path.join(HERE, "golden", "camera_ref.npz"), allow_pickle=False)
    bb, nk = _camera()
    n, h, w = CC.GOLDEN_SIZES[case]
    feats = bb(CC.images(100 + case, n, h, w).to(DEV))
    necks = nk(feats)
    tol = 2 * float(g[f"c{case}_fp32_err"]) + 1e-4
    for li, t in enumerate(feats):
        check_summary(g, f"c{case}_bb{li}", t, 10 * case + li, 2e-6, tol)
    for li, t in enumerate(necks):
        check_summary(g, f"c{case}_neck{li}", t, 10 * case + 5 + li, 2e-6, tol)


def test_full_size_against_float64_restatement():
    """6 x 3 x 384 x 1056: the HIP error stays within 2x the float32 restatement's error + 1e-4"""
    bb, nk = _camera()
    img = CC.images(7, 6, 384, 1056).to(DEV)
    got = list(bb(img))
    got += list(nk(got))
    sd64 = CC.cast(bb.state_dict(), torch.float64, DEV)
    nd64 = CC.cast(nk.state_dict(), torch.float64, DEV)
    sd32 = CC.cast(bb.state_dict(), torch.float32, DEV)
    nd32 = CC.cast(nk.state_dict(), torch.float32, DEV)
    with torch.no_grad():
        f64 = CC.swin_forward(sd64, img.double())
        ref = f64 + list(CC.neck_forward(nd64, f64))
        del f64
        f32 = CC.swin_forward(sd32, img)
        r32 = f32 + list(CC.neck_forward(nd32, f32))
    assert [tuple(t.shape) for t in got] == [(6, 192, 48, 132), (6, 384, 24, 66), (6, 768, 12, 33),
                                             (6, 256, 48, 132), (6, 256, 24, 66)]
    for a, b, c in zip(got, ref, r32):
        e_hip = float((a.double() - b).abs().max())
        e_32 = float((c.double() - b).abs().max())
        assert e_hip <= 2 * e_32 + 1e-4, (e_hip, e_32)


# ---------------------------------------------------------------------------------------------------- detector
_DET = {}


def _detector():
    if "det" not in _DET:
        from detector_common import build_path, detector_inputs
        from isfusion_amd import registry
        with open(os.path.join(HERE, "golden", "isfusion_0075voxel_model.txt")) as f:
            model = ast.literal_eval(f.read())
        path = build_path()
        bb, nk = _camera("cpu")
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


def _boxes_equal(a, b):
    for ra, rb in zip(a, b):
        for k in ("boxes_3d", "scores_3d", "labels_3d"):
            assert torch.equal(ra["pts_bbox"][k].cpu(), rb["pts_bbox"][k].cpu()), k


def test_detector_simple_test_equals_pts_path_on_camera_features():
    det, (pts, img, kw, metas) = _detector()
    feats = det.img_neck(det.img_backbone(img.view(-1, 3, 384, 1056)))
    from isfusion_amd.detector import ISFusionPtsPath
    want = ISFusionPtsPath.simple_test(det, pts, [dict(m) for m in metas], feats, **kw)
    m2 = [dict(m) for m in metas]
    got = det.simple_test(pts, m2, img=img.clone(), **kw)
    assert len(got) == len(pts) and got[0]["pts_bbox"]["boxes_3d"].shape[0] > 0
    _boxes_equal(got, want)
    assert all(tuple(m["input_shape"]) == (384, 1056) for m in m2)
    # forward_test with one augmentation dispatches to simple_test
    _boxes_equal(det.forward_test([pts], [[dict(m) for m in metas]], [img.clone()], **kw), want)


def test_img_mask_idx_zeroes_cameras():
    det, (pts, img, kw, metas) = _detector()
    x = img.clone()
    m = [dict(metas[0], img_mask_idx=[1, 4]), dict(metas[1], img_mask_idx=[-1])]
    got = det.extract_img_feat(x, m)
    ref_img = img.clone()
    ref_img[0, [1, 4]] = 0.0
    want = det.img_neck(det.img_backbone(ref_img.view(-1, 3, 384, 1056)))
    assert torch.equal(x, ref_img)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_aug_test_runs_the_camera_branch_once_per_frame():
    from isfusion_amd.input_pipeline import flip_tta_views
    det, (pts, img, kw, metas) = _detector()
    m = dict(metas[0], lidar_aug_matrix=kw["lidar_aug_matrix"][0].numpy())
    vp, vm = flip_tta_views(pts[0].cpu().numpy(), m, pcd_vertical_flip=False)
    vpts = [torch.from_numpy(p).to(DEV) for p in vp]
    args = dict(lidar2img=kw["lidar2img"][:1], img_aug_matrix=kw["img_aug_matrix"][:1])
    calls = []
    hook = det.img_backbone.register_forward_hook(lambda *a: calls.append(1))
    try:
        got = det.aug_test(vpts, [dict(x) for x in vm], img[:1].clone(), **args)
    finally:
        hook.remove()
    assert len(calls) == 1
    feats = det.img_neck(det.img_backbone(img[0]))
    from isfusion_amd.detector import ISFusionPtsPath
    want = ISFusionPtsPath.aug_test(det, vpts, [dict(x) for x in vm], feats, **args)
    _boxes_equal(got, want)


def test_extract_img_feat_makes_no_host_sync():
    det, (pts, img, kw, metas) = _detector()
    x = img.clone()
    det.extract_img_feat(x, [dict(m) for m in metas])     # packs the weights
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = det.extract_img_feat(x, [dict(m, img_mask_idx=[2]) for m in metas])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(torch.isfinite(t).all() for t in out)


def test_camera_branch_is_bit_identical_run_to_run():
    det, (pts, img, kw, metas) = _detector()
    a = det.extract_img_feat(img.clone(), [dict(m) for m in metas])
    b = det.extract_img_feat(img.clone(), [dict(m) for m in metas])
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_state_dict_round_trip_repacks():
    from isfusion_amd import registry
    det, (pts, img, kw, metas) = _detector()
    before = det.extract_img_feat(img.clone(), [dict(m) for m in metas])
    with open(os.path.join(HERE, "golden", "isfusion_0075voxel_model.txt")) as f:
        model = ast.literal_eval(f.read())
    other = registry.build_detector({"model": model}).to(DEV).eval()
    other.load_state_dict(det.state_dict(), strict=True)
    after = other.extract_img_feat(img.clone(), [dict(m) for m in metas])
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    # new weights in place: the packed copies are re-derived
    sd = det.img_neck.state_dict()
    sd["fpn_convs.0.bn.bias"] = sd["fpn_convs.0.bn.bias"] + 1.0
    other.img_neck.load_state_dict(sd, strict=True)
    changed = other.extract_img_feat(img.clone(), [dict(m) for m in metas])
    assert not torch.equal(changed[0], before[0]) and torch.equal(changed[1], before[1])
