"""GPU tests of the camera branch's training path (isf_swin_gemm_rowscale, isf_swin_train.hip, SwinTransformer /
GeneralizedLSSFPN.forward_train, ISFusionDetector.forward_train): every new kernel and both modules against float64
torch (tests/camera_train_common.py) on the smallest shapes at which they can still go wrong.

Tolerance, the camera branch's convention (tests/test_gpu_camera.py): err(HIP vs float64) <= 2 x err(float32 stock torch,
same inputs, same GPU, vs float64) + floor, with floor = 2e-6 x max|ref| for single kernels and 1e-4 for whole modules."""
import ast
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import camera_common as CC
import camera_train_common as CT
from test_camera import BACKBONE_SEED, NECK_SEED

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return lambda *shape, s=1.0: (torch.randn(*shape, generator=g, dtype=torch.float64) * s).to(DEV)


def _packed(w):
    from isfusion_amd.fusion_ops import PackedLinear
    return PackedLinear(w.float().contiguous())


def _within(name, got, ref, f32, floor_rel=None, floor_abs=None):
    """the convention above; prints the figures before it asserts"""
    ref = ref.double()
    e_hip = float((got.double() - ref).abs().max())
    e_32 = float((f32.double() - ref).abs().max())
    top = float(ref.abs().max())
    floor = floor_rel * top if floor_rel is not None else floor_abs
    print(f"{name}: max|ref| {top:.3e} err hip {e_hip:.3e} err f32 {e_32:.3e} bound {2 * e_32 + floor:.3e}")
    assert e_hip <= 2 * e_32 + floor, (name, e_hip, e_32, top)


# -------------------------------------------------------------------------------------------- 1. row-scale epilogue
@pytest.mark.parametrize("shape", [(3, 5, 7, 96, 96), (3, 5, 7, 384, 96), (2, 9, 15, 96, 96)])
def test_rowscale_epilogue(shape):
    """105 rows: three samples inside one 128-row tile; 270 rows: a sample boundary inside a tile"""
    from isfusion_amd import _lib, swin
    B, H, W, K, N = shape
    M = B * H * W
    r = _gen(B * H * W + K)
    x, w, b, res = r(M, K), r(N, K, s=K ** -0.5), r(N, s=0.1), r(M, N)
    keep = torch.tensor([1.0, 0.0, 1.0][:B], dtype=torch.float64, device=DEV)
    scale = keep / 0.8
    xf, rf = x.float().contiguous(), res.float().contiguous()
    pl = _packed(w)
    got = swin.gemm(swin._a(_lib.SWIN_A_ROWS, xf, ldx=K), M, K, pl, shift=b.float(), residual=rf,
                    row_scale=scale.float().contiguous())
    rows = scale.repeat_interleave(H * W)[:, None]
    ref = F.linear(x, w, b) * rows + res
    f32 = F.linear(xf, w.float(), b.float()) * rows.float() + rf
    _within(f"rowscale {shape}", got, ref, f32, floor_rel=2e-6)
    dropped = (rows == 0).expand_as(ref)
    assert dropped.any() and torch.equal(got[dropped], rf[dropped])           # bit for bit the residual
    ones = torch.ones(B, dtype=torch.float32, device=DEV)
    plain = swin.gemm(swin._a(_lib.SWIN_A_ROWS, xf, ldx=K), M, K, pl, shift=b.float(), residual=rf)
    assert torch.equal(swin.gemm(swin._a(_lib.SWIN_A_ROWS, xf, ldx=K), M, K, pl, shift=b.float(), residual=rf,
                                 row_scale=ones), plain)


# ------------------------------------------------------------------------------------- 2. backward of the lateral step
LATERAL = [(2, (7, 9), (4, 5), 64, 96, 64),        # 126 rows < one tile, ratio not 2
           (3, (12, 22), (6, 11), 192, 256, 256),  # 792 rows, image boundaries inside tiles, shipped level-0 channels
           (1, (6, 8), (3, 4), 384, 768, 256),     # shipped level-1 channels
           (2, (1, 8), (1, 3), 64, 96, 64),        # h == 1: scale 0 along y
           (2, (5, 6), (5, 6), 64, 96, 64)]        # h2 == h


def _lateral_torch(fine, coarse, w, g):
    """(up^T g as NCHW, dW, dcoarse) by autograd over F.interpolate + cat + conv2d(1x1), in the inputs' dtype"""
    coarse = coarse.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    up = F.interpolate(coarse, size=fine.shape[2:], mode="bilinear", align_corners=True)
    y = F.conv2d(torch.cat([fine, up], 1), w)
    dw, dc = torch.autograd.grad(y, (w, coarse), g)
    probe = torch.zeros(coarse.shape[0], g.shape[1], *coarse.shape[2:], dtype=g.dtype, device=g.device, requires_grad=True)
    upt, = torch.autograd.grad(F.interpolate(probe, size=fine.shape[2:], mode="bilinear", align_corners=True), probe, g)
    return upt, dw, dc


@pytest.mark.parametrize("case", range(len(LATERAL)))
@pytest.mark.parametrize("log2_scale", [0, -20, 10])
def test_lateral_backward(case, log2_scale):
    from isfusion_amd import generalized_lss as gl
    B, (H, W), (H2, W2), C1, C2, N = LATERAL[case]
    r = _gen(1000 + case)
    fine, coarse, w = r(B, C1, H, W), r(B, C2, H2, W2), r(N, C1 + C2, 1, 1, s=(C1 + C2) ** -0.5)
    g = r(B, N, H, W) * 2.0 ** log2_scale
    ref = _lateral_torch(fine, coarse, w, g)
    f32 = _lateral_torch(fine.float(), coarse.float(), w.float(), g.float())

    def run():
        c = coarse.float().requires_grad_(True)
        wf = w.float().requires_grad_(True)
        rows = gl.LateralFunction.apply(fine.float(), c, wf)
        grows = g.float().permute(0, 2, 3, 1).reshape(B * H * W, N).contiguous()
        dc, dw = torch.autograd.grad(rows, (c, wf), grows)
        upt = gl.upsample_rows_adjoint(grows, B, H, W, H2, W2).view(B, H2, W2, N).permute(0, 3, 1, 2)
        return rows, upt, dw, dc

    rows, upt, dw, dc = run()
    y64 = F.conv2d(torch.cat([fine, F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)], 1), w)
    assert float((rows.view(B, H, W, N).permute(0, 3, 1, 2).double() - y64).abs().max()) < 1e-5 * float(y64.abs().max())
    tag = f"lateral {LATERAL[case]} 2^{log2_scale}"
    _within(tag + " upT", upt, ref[0], f32[0], floor_rel=2e-6)
    _within(tag + " dW", dw, ref[1], f32[1], floor_rel=2e-6)
    _within(tag + " dcoarse", dc, ref[2], f32[2], floor_rel=2e-6)
    again = run()
    for a, b in zip((rows, upt, dw, dc), again):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- 3. dW kernel alone
@pytest.mark.parametrize("R,B,hw", [(130, 2, 65), (2 * 2048 + 7, 11, 373)])
@pytest.mark.parametrize("NK", [(256, 192), (64, 1152)])
def test_rows_weight_grad(R, B, hw, NK):
    """several chunks and a ragged tail; X as token rows and as an NCHW map (odd hw: unaligned 8-row groups, groups
    that straddle two images)"""
    from isfusion_amd import _lib, generalized_lss as gl
    N, K = NK
    assert B * hw == R and _lib.load().isf_rows_weight_grad_chunks(R, N, K) > 1
    r = _gen(R + N)
    g, x = r(R, N), r(R, K)
    ref = g.t() @ x
    f32 = g.float().t() @ x.float()
    gs, sc = _lib.grad_rescale(g.float())
    xr = x.float().contiguous()
    xm = x.float().view(B, hw, K).permute(0, 2, 1).contiguous().view(B, K, 1, hw)
    for name, xx in (("rows", xr), ("nchw", xm)):
        got = gl.rows_weight_grad(gs, xx, sc[1:])
        _within(f"dW {name} R={R} {NK}", got, ref, f32, floor_rel=2e-6)
        assert torch.equal(got, gl.rows_weight_grad(gs, xx, sc[1:]))
    # into a column block of a wider matrix
    wide = torch.full((N, K + 32), 7.0, dtype=torch.float32, device=DEV)
    gl.rows_weight_grad(gs, xr, sc[1:], out=wide[:, 32:])
    assert torch.equal(wide[:, 32:], gl.rows_weight_grad(gs, xr, sc[1:])) and bool((wide[:, :32] == 7.0).all())


# --------------------------------------------------------------------------------------- 4. backbone forward_train
def _backbone(drop_path_rate=None):
    from isfusion_amd.swin import SwinTransformer
    cfg = dict(CC.BACKBONE)
    if drop_path_rate is not None:
        cfg["drop_path_rate"] = drop_path_rate
    bb = SwinTransformer(**cfg)
    bb.load_state_dict(CC.seeded_module_state(bb, BACKBONE_SEED))
    return bb.to(DEV)


def test_backbone_forward_train_equals_float64():
    bb = _backbone().train()
    n, h, w = 3, 90, 150
    img = CC.images(31, n, h, w).to(DEV)
    keep = CT.fixed_drop_keep(32, n).to(DEV)
    got = bb.forward_train(img, drop_keep=keep)
    assert all(not t.requires_grad for t in got)
    with torch.no_grad():
        ref = CT.swin_forward_train(CC.cast(bb.state_dict(), torch.float64, DEV), img.double(), keep)
        f32 = CT.swin_forward_train(CC.cast(bb.state_dict(), torch.float32, DEV), img, keep)
        ev = CC.swin_forward(CC.cast(bb.state_dict(), torch.float64, DEV), img.double())
    assert [tuple(t.shape) for t in got] == [tuple(t.shape) for t in ref]
    assert float((ev[0] - ref[0]).abs().max()) > 1e-2          # the masks matter
    for i, (a, b, c) in enumerate(zip(got, ref, f32)):
        _within(f"backbone map {i}", a, b, c, floor_abs=1e-4)


def test_backbone_forward_train_without_drop_path_equals_eval():
    bb = _backbone(0.0)
    img = CC.images(33, 3, 90, 150).to(DEV)
    assert bb.drop_layers() == []
    a = bb.train().forward_train(img)
    b = bb.eval()(img)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_backbone_forward_train_draws_from_the_torch_seed():
    bb = _backbone().train()
    img = CC.images(34, 3, 90, 150).to(DEV)
    with _rng_restored():
        torch.manual_seed(5)
        a = bb.forward_train(img)
        torch.manual_seed(5)
        b = bb.forward_train(img)
        torch.manual_seed(6)
        c = bb.forward_train(img)
    assert all(torch.equal(x, y) and not x.requires_grad for x, y in zip(a, b))
    assert any(not torch.equal(x, y) for x, y in zip(a, c))
    with pytest.raises(ValueError):
        bb.forward_train(img, drop_keep=torch.ones(3, 3, device=DEV))


# ------------------------------------------------------------------------------------------- 5. neck forward_train
NECK_GRIDS = ((12, 22), (6, 11), (3, 6))
_NECK = {}


def _neck_case():
    """inputs, upstream gradients and the float64 / float32 references, computed once"""
    if _NECK:
        return _NECK
    from isfusion_amd.generalized_lss import GeneralizedLSSFPN
    nk = GeneralizedLSSFPN(**CC.NECK)
    sd = CC.seeded_module_state(nk, NECK_SEED)
    r = _gen(500)
    feats = [r(2, c, h, w) for c, (h, w) in zip(CC.NECK["in_channels"], NECK_GRIDS)]
    # upstream gradients of about 1 / sqrt(elements): parameter gradients of order 1, where the 1e-4 floor means something
    ups = [CT.upstream(600 + i, (2, 256, h, w)).to(DEV) / (2 * h * w) ** 0.5 for i, (h, w) in enumerate(NECK_GRIDS[:2])]
    _NECK.update(sd=sd, feats=feats, ups=ups, refs={})
    for both in (True, False):
        for dtype in (torch.float64, torch.float32):
            p = CT.leaf_params(sd, dtype, DEV)
            outs = CT.neck_forward_train(p, [f.to(dtype) for f in feats])
            loss = (outs[1] * ups[1].to(dtype)).sum() + ((outs[0] * ups[0].to(dtype)).sum() if both else 0.0)
            loss.backward()
            _NECK["refs"][both, dtype] = ([o.detach() for o in outs], p)
    return _NECK


@pytest.mark.parametrize("both", [True, False])
def test_neck_forward_train_outputs_gradients_and_statistics(both):
    from isfusion_amd.generalized_lss import GeneralizedLSSFPN
    case = _neck_case()
    nk = GeneralizedLSSFPN(**CC.NECK)
    nk.load_state_dict(case["sd"])
    nk = nk.to(DEV).train()
    outs = nk.forward_train([f.float() for f in case["feats"]])
    ups = case["ups"]
    loss = (outs[1] * ups[1].float()).sum() + ((outs[0] * ups[0].float()).sum() if both else 0.0)
    loss.backward()
    (o64, p64), (o32, p32) = case["refs"][both, torch.float64], case["refs"][both, torch.float32]
    for i in range(2):
        assert tuple(outs[i].shape) == tuple(o64[i].shape)
        assert outs[i].permute(0, 2, 3, 1).is_contiguous()            # an NCHW view of token rows
        _within(f"neck out {i}", outs[i].detach(), o64[i], o32[i], floor_abs=1e-4)
    for name, p in nk.named_parameters():
        if not both and name.startswith(("lateral_convs.0.", "fpn_convs.0.")):
            assert p.grad is None and p64[name].grad is None, name
            continue
        assert p.grad is not None and p.grad.dtype == torch.float32, name
        _within(f"neck grad {name}", p.grad, p64[name].grad, p32[name].grad, floor_abs=1e-4)
    bns = 0
    for name, b in nk.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(b) == 1 == int(p64[name])
            bns += 1
        else:
            _within(f"neck {name}", b, p64[name], p32[name], floor_abs=1e-4)
    assert bns == 4


def test_neck_forward_train_refuses_inputs_with_grad_and_runs_under_autocast():
    from isfusion_amd.generalized_lss import GeneralizedLSSFPN
    case = _neck_case()
    nk = GeneralizedLSSFPN(**CC.NECK)
    nk.load_state_dict(case["sd"])
    nk = nk.to(DEV).train()
    feats = [f.float() for f in case["feats"]]
    with pytest.raises(NotImplementedError, match="backward"):
        nk.forward_train([feats[0], feats[1].clone().requires_grad_(True), feats[2]])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        outs = nk.forward_train(feats)
        loss = (outs[1].float() * case["ups"][1].float()).sum()
    loss.backward()
    for name, p in nk.named_parameters():
        if name.startswith(("lateral_convs.1.", "fpn_convs.1.")):
            assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), name


# ----------------------------------------------------------------------------------------------------- 6. detector
_DET = {}


def _build_detector():
    from detector_common import build_path
    from isfusion_amd import head_loss, registry
    from test_camera import _modules
    with open(os.path.join(HERE, "golden", "isfusion_0075voxel_model.txt")) as f:
        model = ast.literal_eval(f.read())
    path = build_path()
    bb, nk = _modules()
    det = registry.build_detector({"model": model})
    sd = dict(path.state_dict())
    sd.update({"img_backbone." + k: v for k, v in CC.seeded_module_state(bb, BACKBONE_SEED).items()})
    sd.update({"img_neck." + k: v for k, v in CC.seeded_module_state(nk, NECK_SEED).items()})
    det.load_state_dict(sd, strict=True)
    det.pts_bbox_head.train_cfg = dict(head_loss.SHIPPED_TRAIN_CFG)
    return det.to(DEV)


def _detector():
    if not _DET:
        from detector_common import detector_inputs
        from isfusion_amd import synthetic
        det = _build_detector()
        pts, inp, kw, metas = detector_inputs()
        img = CC.images(11, 6 * len(pts), 384, 1056).view(len(pts), 6, 3, 384, 1056).to(DEV)
        scenes = [synthetic.scene_boxes(4321 + i) for i in range(len(pts))]
        _DET.update(det=det, start={k: v.detach().clone() for k, v in det.state_dict().items()},
                    pts=[torch.from_numpy(p).to(DEV) for p in pts], img=img, kw=kw, metas=metas,
                    gtb=[torch.from_numpy(b).to(DEV) for b, _ in scenes],
                    gtl=[torch.from_numpy(l).to(DEV) for _, l in scenes])
    return _DET


class _rng_restored:
    """the process-wide generators (torch, random, numpy) back as they were when the block ends: what the detector test
    seeds must not reach the tests that run after it"""

    def __enter__(self):
        self.state = (torch.get_rng_state(), torch.cuda.get_rng_state_all(), random.getstate(), np.random.get_state())

    def __exit__(self, *exc):
        torch.set_rng_state(self.state[0])
        torch.cuda.set_rng_state_all(self.state[1])
        random.setstate(self.state[2])
        np.random.set_state(self.state[3])
        return False


def _fresh(d):
    """the detector back at its starting weights and BatchNorm buffers, gradients cleared, every generator re-seeded"""
    det = d["det"]
    det.load_state_dict(d["start"], strict=True)
    det.train()
    det.zero_grad(set_to_none=True)
    torch.manual_seed(3)
    random.seed(3)
    np.random.seed(3)
    return det


def _total(ld):
    return sum(v for k, v in ld.items() if k != "matched_ious")


def _neck_grads(det):
    return {n: p.grad.detach().clone() for n, p in det.img_neck.named_parameters() if p.grad is not None}


def _hand_chained(d):
    """extract_img_feat's output as a leaf -> ISFusionPtsPath.forward_train -> the leaf's gradient pushed through the
    neck's graph by hand"""
    from isfusion_amd.detector import ISFusionPtsPath
    det = _fresh(d)
    feats = det.extract_img_feat(d["img"].clone(), [dict(m) for m in d["metas"]])
    leaf = [f.detach().requires_grad_(True) for f in feats]
    ld = ISFusionPtsPath.forward_train(det, d["pts"], leaf, [dict(m, input_shape=(384, 1056)) for m in d["metas"]],
                                       d["gtb"], d["gtl"], **d["kw"])
    _total(ld).backward()
    assert leaf[0].grad is None and leaf[1].grad is not None          # only the stride-16 map reaches Point-to-Grid
    feats[1].backward(leaf[1].grad)
    return ld, _neck_grads(det)


MAX_ROUNDS = 4             # rounds of (two hand-chained steps, one detector step) at most
SAME_OUTCOME = 1e-6        # relative loss_heatmap distance of "the same outcome": float32 summation-order noise of a loss
                           # is a few ulps (6e-8 each); a discrete flip upstream moves it by orders of magnitude more


def test_detector_forward_train():
    """Loss dict, gradients where the shipped model has them, and the detector's img_neck gradients against the
    hand-chained composition (extract_img_feat's output as a leaf -> ISFusionPtsPath.forward_train -> the leaf's gradient
    pushed through img_neck.forward_train by hand): at most 10 x the spread between two identical hand-chained steps
    + 1e-6, relative to the tensor's largest entry.  The points path's own forward makes a discrete choice that is not
    reproducible run to run, so identical steps land in one of a few outcomes, told apart by
    loss_heatmap; steps are repeated until a detector step and two hand-chained steps share one, the spread is measured
    between those two and the detector step is compared with the first of them.  Measured spread on an MI355X: 0.65e-2 - 2e-2 of the largest entry
    inside one outcome (0.35 between two).  Extra: the gradient captured at the stride-16 map in the detector's own step,
    pushed by hand through a repeated camera forward, reproduces the detector's gradients (measured difference 0)."""
    with _rng_restored():
        try:
            _detector_forward_train()
        finally:
            _DET.clear()             # the detector, its images and its starting state: nothing later uses them


def _detector_step(d):
    """one step through ISFusionDetector.forward_train -> (loss dict, img_neck gradients, the gradient that arrived at
    the stride-16 map, the detector)"""
    det = _fresh(d)
    metas = [dict(m) for m in d["metas"]]
    seen = {}
    real = det.extract_img_feat

    def spy(img, img_metas):
        feats = real(img, img_metas)
        feats[1].register_hook(lambda g: seen.__setitem__("grad", g.detach().clone()))
        return feats

    det.extract_img_feat = spy
    try:
        ld = det.forward_train(points=d["pts"], img_metas=metas, gt_bboxes_3d=d["gtb"], gt_labels_3d=d["gtl"],
                               img=d["img"].clone(), **d["kw"])
    finally:
        del det.extract_img_feat
    assert all(tuple(m["input_shape"]) == (384, 1056) for m in metas)
    _total(ld).backward()
    return ld, _neck_grads(det), seen["grad"], det


def _same_outcome(x, y):
    x, y = float(x["loss_heatmap"]), float(y["loss_heatmap"])
    return abs(x - y) <= SAME_OUTCOME * abs(x)


def _detector_forward_train():
    from isfusion_amd.detector import ISFusionPtsPath
    d = _detector()
    ld, got, arrived, det = _detector_step(d)
    assert set(ld) == {"loss_heatmap", "loss_heatmap_ins", "layer_-1_loss_cls", "layer_-1_loss_bbox", "matched_ious"}
    assert all(bool(torch.isfinite(v).all()) for v in ld.values())
    for name, p in det.named_parameters():
        if name.startswith("img_backbone."):
            assert p.grad is None, name
        elif name.startswith(("img_neck.lateral_convs.1.", "img_neck.fpn_convs.1.")):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
        elif name.startswith("img_neck."):
            assert p.grad is None, name
    assert len(got) == 6
    # extra: the gradient that arrived in the detector's own step, pushed by hand through a repeated camera forward
    det = _fresh(d)
    feats = det.extract_img_feat(d["img"].clone(), [dict(m) for m in d["metas"]])
    feats[1].backward(arrived)
    pushed = _neck_grads(det)
    assert sorted(pushed) == sorted(got)
    for name in sorted(got):
        err = float((got[name] - pushed[name]).abs().max()) / float(got[name].abs().max())
        print(f"detector {name}: captured gradient pushed by hand vs detector {err:.3e}")
        assert err <= 1e-6, (name, err)
    # the issue's check: rounds of (two hand-chained steps, one detector step) until a detector step and two
    # hand-chained steps share an outcome
    dets, hands, pick = [(ld, got)], [], None
    for rnd in range(MAX_ROUNDS):
        hands += [_hand_chained(d), _hand_chained(d)]
        if rnd:
            dets.append(_detector_step(d)[:2])
        for l, _ in hands[-2:] + dets[-1:]:
            print(f"round {rnd}:", {k: round(float(v), 5) for k, v in l.items()})
        for dl, dg in dets:
            mates = [h for hl, h in hands if _same_outcome(dl, hl)]
            if len(mates) >= 2:
                pick = (dg, mates[0], mates[1])
        if pick:
            break
    assert all(set(hl) == set(ld) and sorted(h) == sorted(got) for hl, h in hands)
    assert pick, f"no detector step shared its outcome with two hand-chained steps in {MAX_ROUNDS} rounds"
    got, a, b = pick
    for name in sorted(got):
        top = float(a[name].abs().max())
        spread = float((a[name] - b[name]).abs().max()) / top
        err = float((got[name] - a[name]).abs().max()) / top
        print(f"detector {name}: max|grad| {top:.3e} spread {spread:.3e} detector vs hand-chained {err:.3e} "
              f"(10 x spread + 1e-6 = {10 * spread + 1e-6:.3e})")
        assert err <= 10 * spread + 1e-6, (name, err, spread)
    det = _fresh(d)
    # detach=False has no backward to offer
    det.detach = False
    try:
        with pytest.raises(NotImplementedError, match="Swin"):
            det.extract_img_feat(d["img"].clone(), [dict(m) for m in d["metas"]])
    finally:
        det.detach = True
    # eval after training: the moved BatchNorm buffers are repacked; a fresh detector with the same state agrees
    det.eval()
    out = det.simple_test(d["pts"], [dict(m) for m in d["metas"]], img=d["img"].clone(), **d["kw"])
    other = _build_detector()
    other.load_state_dict(det.state_dict(), strict=True)
    want = other.eval().simple_test(d["pts"], [dict(m) for m in d["metas"]], img=d["img"].clone(), **d["kw"])
    assert len(out) == len(d["pts"])
    for ra, rb in zip(out, want):
        for k in ("boxes_3d", "scores_3d", "labels_3d"):
            assert torch.equal(ra["pts_bbox"][k].cpu(), rb["pts_bbox"][k].cpu()), k
    assert isinstance(det, ISFusionPtsPath)
