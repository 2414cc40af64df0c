"""Time the camera branch on one GPU (device events, after warm-up) at B = 2 samples x 6 cameras x 384 x 1056:
  * SwinTransformer, GeneralizedLSSFPN and ISFusionDetector.extract_img_feat on the HIP kernels (isf_swin.hip,
    dense_conv.py)
  * the same backbone and neck as the float32 stock-torch composition (tests/camera_common.py: conv2d, layer_norm,
    linear, roll / window copies, softmax, interpolate, conv2d + batch_norm) on the same GPU and weights
  * ISFusionDetector.simple_test (images -> boxes) against ISFusionPtsPath.simple_test on precomputed camera features

    python tools/camera_bench.py [--steps 10] [--warmup 3] [--points 300000]
    python tools/camera_bench.py --train [--backward] [--steps 10] [--warmup 3] [--runs 3]
    python tools/camera_bench.py --precision both [--steps 10] [--warmup 3] [--runs 3]
    python tools/camera_bench.py --train [--backward] --precision mixed [--steps 5] [--warmup 2] [--runs 3]

--precision f32 (default) is the run above.  f16 / both: the backbone's precision modes (SwinTransformer.set_precision)
in ONE process on the same weights and images -- per run and mode the backbone, extract_img_feat and
ISFusionDetector.simple_test times, and once per mode the error of the three backbone maps against the float64
restatement at the bench size.

--train: one camera training step instead -- SwinTransformer.forward_train (stochastic depth, no backward: detach=True)
+ GeneralizedLSSFPN.forward_train + the neck's backward from a gradient on the stride-16 output (what Point-to-Grid
sends back), against the float32 stock-torch composition of tests/camera_train_common.py (same masks, autograd) on the
same GPU, each measured --runs times; plus the single kernels of the lateral step's backward at the shipped level-1 size.
--train --backward: the step with the backbone's backward as well (ISFusionDetector.camera_backward), against stock-torch
autograd over backbone and neck, --runs times each, and the peak memory each step adds.
--train [--backward] --precision mixed: the HIP step in the f32 mode and in the mixed-precision training mode
(SwinTransformer.set_precision("mixed")), one after the other in ONE process on the same weights, images and masks; the
rows carry a "precision" field.

Prints one JSON line per measurement (ms per call, mean over --steps)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import camera_common as CC  # noqa: E402
from isfusion_amd import synthetic  # noqa: E402
from isfusion_amd.detector import ISFusionDetector, ISFusionPtsPath  # noqa: E402
from isfusion_amd.fusion_modules import seeded_state_dict  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def train_bench(a, dev):
    import camera_train_common as CT
    from isfusion_amd import _lib, generalized_lss as gl
    from isfusion_amd.generalized_lss import GeneralizedLSSFPN
    from isfusion_amd.swin import SwinTransformer
    bb, nk = SwinTransformer(**CC.BACKBONE), GeneralizedLSSFPN(**CC.NECK)
    bb.load_state_dict(CC.seeded_module_state(bb, 4101))
    nk.load_state_dict(CC.seeded_module_state(nk, 4202))
    bb, nk = bb.to(dev).train(), nk.to(dev).train()
    B, H, W = 2, 384, 1056
    flat = CC.images(3, B * 6, H, W).to(dev)
    keep = CT.fixed_drop_keep(9, B * 6).to(dev)
    up = torch.randn(B * 6, 256, H // 16, W // 16, device=dev) * 1e-3

    def hip_step():
        for p in nk.parameters():
            p.grad = None
        outs = nk.forward_train(bb.forward_train(flat, drop_keep=keep))
        outs[1].backward(up)

    sd = CC.cast(bb.state_dict(), torch.float32, dev)
    nd = CT.leaf_params(nk.state_dict(), torch.float32, dev)

    def torch_step():
        for v in nd.values():
            v.grad = None
        with torch.no_grad():
            feats = CT.swin_forward_train(sd, flat, keep)
        outs = CT.neck_forward_train(nd, feats)
        outs[1].backward(up)

    if a.backward:
        return train_backward_bench(a, bb, nk, flat, keep, up, sd, nd)
    for run in range(a.runs):
        for mode in train_modes(a):
            bb.set_precision(mode)
            ms = timed(hip_step, a.steps, a.warmup)
            print(json.dumps(dict(what="camera_train_step", impl="hip", precision=mode, images=B * 6, hw=[H, W], run=run,
                                  ms=round(ms, 3))))
        bb.set_precision("f32")
        ms = timed(torch_step, a.steps, a.warmup)
        print(json.dumps(dict(what="camera_train_step", impl="torch_fp32", images=B * 6, hw=[H, W], run=run,
                              ms=round(ms, 3))))
    ms = timed(lambda: bb.forward_train(flat, drop_keep=keep), a.steps, a.warmup)
    print(json.dumps(dict(what="backbone_forward_train", impl="hip", images=B * 6, ms=round(ms, 3))))
    with torch.no_grad():
        ms = timed(lambda: CT.swin_forward_train(sd, flat, keep), a.steps, a.warmup)
    print(json.dumps(dict(what="backbone_forward_train", impl="torch_fp32", images=B * 6, ms=round(ms, 3))))
    feats = bb.forward_train(flat, drop_keep=keep)

    def neck_hip():
        for p in nk.parameters():
            p.grad = None
        nk.forward_train(feats)[1].backward(up)

    def neck_torch():
        for v in nd.values():
            v.grad = None
        CT.neck_forward_train(nd, feats)[1].backward(up)

    print(json.dumps(dict(what="neck_forward_backward", impl="hip", ms=round(timed(neck_hip, a.steps, a.warmup), 3))))
    print(json.dumps(dict(what="neck_forward_backward", impl="torch_fp32",
                          ms=round(timed(neck_torch, a.steps, a.warmup), 3))))
    # the lateral step's backward kernels at the shipped level-1 size: fine 24 x 66 x 384, coarse 12 x 33 x 768, N = 256
    n, (h, w), (h2, w2) = B * 6, (H // 16, W // 16), (H // 32, W // 32)
    g, sc = _lib.grad_rescale(up.permute(0, 2, 3, 1).reshape(n * h * w, 256).contiguous())
    fine, coarse = feats[1], feats[2]
    g2 = gl.upsample_rows_adjoint(g, n, h, w, h2, w2)
    for what, fn in (("upsample_rows_adjoint", lambda: gl.upsample_rows_adjoint(g, n, h, w, h2, w2)),
                     ("rows_weight_grad fine [R 19008, N 256, K 384]", lambda: gl.rows_weight_grad(g, fine, sc[1:])),
                     ("rows_weight_grad coarse [R 4752, N 256, K 768]", lambda: gl.rows_weight_grad(g2, coarse, sc[1:])),
                     ("torch fp32 g^T x fine (rows)", lambda: g.t().matmul(fine.permute(0, 2, 3, 1).reshape(-1, 384)))):
        print(json.dumps(dict(what=what, ms=round(timed(fn, a.steps * 5, a.warmup), 4))))


def train_modes(a):
    """--train: the backbone's precision modes to time, in one process"""
    return ("f32", "mixed") if a.precision == "mixed" else ("f32",)


def train_backward_bench(a, bb, nk, flat, keep, up, sd, nd):
    """--train --backward: backbone forward with DropPath + neck forward + both backwards from a gradient on the stride-16
    map, next to float32 stock-torch autograd over the same modules and masks; and the peak memory either step adds to
    what is resident before it"""
    import camera_train_common as CT
    n, (H, W) = flat.shape[0], flat.shape[-2:]

    def clear(params):
        for p in params:
            p.grad = None

    def hip_step():
        clear(list(bb.parameters()) + list(nk.parameters()))
        outs = nk.forward_train(bb.forward_train(flat, drop_keep=keep, backward=True), input_grads=True)
        outs[1].backward(up)

    bd = CT.leaf_params(sd, torch.float32, flat.device)

    def torch_step():
        clear(list(bd.values()) + list(nd.values()))
        outs = CT.neck_forward_train(nd, CT.swin_forward_train(bd, flat, keep))
        outs[1].backward(up)

    if a.profile_backward:
        bb.set_precision(a.precision)
        for _ in range(a.warmup + a.steps):
            hip_step()
        torch.cuda.synchronize()
        return
    cases = [("hip", mode, hip_step) for mode in train_modes(a)] + [("torch_fp32", "f32", torch_step)]
    for run in range(a.runs):
        for impl, mode, fn in cases:
            bb.set_precision(mode)
            ms = timed(fn, a.steps, a.warmup)
            print(json.dumps(dict(what="camera_train_step_backward", impl=impl, precision=mode, images=n, hw=[H, W],
                                  run=run, ms=round(ms, 3))))
    for impl, mode, fn in cases:
        bb.set_precision(mode)
        fn()                                  # this mode's packed weights and gradients are resident before the measurement
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        print(json.dumps(dict(what="camera_train_step_backward_peak_memory", impl=impl, precision=mode,
                              mib_over_resident=round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1))))
    bb.set_precision("f32")

    def hip_forward_only():
        outs = nk.forward_train(bb.forward_train(flat, drop_keep=keep))
        outs[1].backward(up)

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    hip_forward_only()
    torch.cuda.synchronize()
    print(json.dumps(dict(what="camera_train_step_peak_memory", impl="hip", note="backward off",
                          mib_over_resident=round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1))))


def build_detector(dev):
    det = ISFusionDetector(img_backbone=dict(type="SwinTransformer", **CC.BACKBONE),
                           img_neck=dict(type="GeneralizedLSSFPN", **CC.NECK), detach=True).eval()
    det._lidar.randomize_weights_(0).randomize_bn_(1)
    for name, seed in (("fusion_encoder", 100), ("pts_backbone", 200), ("pts_neck", 250), ("pts_bbox_head", 300)):
        getattr(det, name).load_state_dict(seeded_state_dict(getattr(det, name), seed))
    det.img_backbone.load_state_dict(CC.seeded_module_state(det.img_backbone, 4101))
    det.img_neck.load_state_dict(CC.seeded_module_state(det.img_neck, 4202))
    det = det.to(dev)
    det.freeze()
    return det


def precision_bench(a, dev):
    modes = ["f32", "f16"] if a.precision == "both" else [a.precision]
    det = build_detector(dev)
    B, H, W = 2, 384, 1056
    img = CC.images(3, B * 6, H, W).to(dev).view(B, 6, 3, H, W)
    flat = img.view(B * 6, 3, H, W)
    bb = det.img_backbone
    pts = [torch.from_numpy(p).to(dev) for p in synthetic.batch(2, B, a.points)]
    inp = synthetic.fusion_inputs(5, B)
    kw = dict(lidar2img=torch.from_numpy(inp["lidar2img"]), img_aug_matrix=torch.from_numpy(inp["img_aug_matrix"]),
              lidar_aug_matrix=torch.from_numpy(inp["lidar_aug_matrix"]))
    metas = [dict(input_shape=inp["input_shape"]) for _ in range(B)]
    with torch.no_grad():
        ref = CC.swin_forward(CC.cast(bb.state_dict(), torch.float64, dev), flat.double())
    for mode in modes:
        det.camera_precision = mode
        got = bb(flat)
        print(json.dumps(dict(what="backbone_error_vs_float64", precision=mode, images=B * 6, hw=[H, W],
                              max_abs_err=[float((x.double() - r).abs().max()) for x, r in zip(got, ref)],
                              max_abs_ref=[float(r.abs().max()) for r in ref])))
    del ref
    for run in range(a.runs):
        for mode in modes:
            det.camera_precision = mode
            row = dict(precision=mode, run=run, images=B * 6)
            print(json.dumps(dict(what="backbone", ms=round(timed(lambda: bb(flat), a.steps, a.warmup), 3), **row)))
            print(json.dumps(dict(what="extract_img_feat",
                                  ms=round(timed(lambda: det.extract_img_feat(img, metas), a.steps, a.warmup), 3), **row)))
            print(json.dumps(dict(what="simple_test", input="images", batch=B,
                                  ms=round(timed(lambda: det.simple_test(pts, metas, img=img, **kw), a.steps, a.warmup), 3),
                                  **row)))
    det.camera_precision = "f32"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--train", action="store_true", help="time one camera training step (forward_train + neck backward)")
    ap.add_argument("--backward", action="store_true",
                    help="with --train: the step with the backbone's backward (forward_train(backward=True), the neck "
                         "with input_grads=True) next to stock-torch autograd over backbone and neck")
    ap.add_argument("--profile-backward", action="store_true",
                    help="with --train --backward: run the HIP step --warmup + --steps times and exit (the process to "
                         "put under a kernel trace)")
    ap.add_argument("--runs", type=int, default=3, help="--train / --precision f16|both: repetitions of the measurement")
    ap.add_argument("--precision", choices=("f32", "f16", "both", "mixed"), default="f32",
                    help="f16 / both: time the backbone's precision modes in one process (default: the f32 run); mixed "
                         "(with --train): the training step in the f32 and the mixed-precision mode in one process")
    ap.add_argument("--profile-forward", action="store_true",
                    help="run the backbone forward of --precision (f32 or f16) --steps times and exit: the process to "
                         "put under a kernel trace (profiles/camera_f16_kernels.txt)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.train:
        if a.precision in ("f16", "both"):
            ap.error("--train times the training modes: --precision f32 or mixed")
        return train_bench(a, dev)
    if a.precision == "mixed":
        ap.error("--precision mixed is a training mode (its eval forward is f16's): use it with --train")
    if a.profile_forward:
        if a.precision == "both":
            ap.error("--profile-forward traces one mode: --precision f32 or f16")
        det = build_detector(dev)
        det.camera_precision = a.precision
        flat = CC.images(3, 12, 384, 1056).to(dev)
        for _ in range(a.warmup + a.steps):
            det.img_backbone(flat)
        torch.cuda.synchronize()
        return None
    if a.precision != "f32":
        return precision_bench(a, dev)
    det = build_detector(dev)
    B, H, W = 2, 384, 1056
    img = CC.images(3, B * 6, H, W).to(dev).view(B, 6, 3, H, W)
    flat = img.view(B * 6, 3, H, W)
    bb, nk = det.img_backbone, det.img_neck
    with torch.no_grad():
        feats = bb(flat)
        necks = nk(feats)
    ms = timed(lambda: bb(flat), a.steps, a.warmup)
    print(json.dumps(dict(what="backbone", impl="hip", images=B * 6, hw=[H, W], ms=round(ms, 3))))
    ms = timed(lambda: nk(feats), a.steps, a.warmup)
    print(json.dumps(dict(what="neck", impl="hip", images=B * 6, ms=round(ms, 3))))
    metas = [dict() for _ in range(B)]
    ms = timed(lambda: det.extract_img_feat(img, metas), a.steps, a.warmup)
    print(json.dumps(dict(what="extract_img_feat", impl="hip", images=B * 6, ms=round(ms, 3))))
    sd = CC.cast(bb.state_dict(), torch.float32, dev)
    nd = CC.cast(nk.state_dict(), torch.float32, dev)
    with torch.no_grad():
        ms_bb = timed(lambda: CC.swin_forward(sd, flat), a.steps, a.warmup)
        ms_nk = timed(lambda: CC.neck_forward(nd, feats), a.steps, a.warmup)
        ref = CC.swin_forward(sd, flat)
        err = max(float((x - y).abs().max()) for x, y in zip(feats, ref))
    print(json.dumps(dict(what="backbone", impl="torch_fp32", images=B * 6, ms=round(ms_bb, 3),
                          max_abs_diff_vs_hip=err)))
    print(json.dumps(dict(what="neck", impl="torch_fp32", images=B * 6, ms=round(ms_nk, 3))))
    print(json.dumps(dict(what="extract_img_feat", impl="torch_fp32", images=B * 6, ms=round(ms_bb + ms_nk, 3),
                          note="backbone + neck")))
    # end to end: images -> boxes, against the point-cloud path on precomputed camera features
    pts = [torch.from_numpy(p).to(dev) for p in synthetic.batch(2, B, a.points)]
    inp = synthetic.fusion_inputs(5, B)
    kw = dict(lidar2img=torch.from_numpy(inp["lidar2img"]), img_aug_matrix=torch.from_numpy(inp["img_aug_matrix"]),
              lidar_aug_matrix=torch.from_numpy(inp["lidar_aug_matrix"]))
    metas = [dict(input_shape=inp["input_shape"]) for _ in range(B)]
    ms = timed(lambda: ISFusionPtsPath.simple_test(det, pts, metas, necks, **kw), a.steps, a.warmup)
    print(json.dumps(dict(what="simple_test", input="camera_features", batch=B, ms=round(ms, 3))))
    ms = timed(lambda: det.simple_test(pts, metas, img=img, **kw), a.steps, a.warmup)
    n = sum(r["pts_bbox"]["scores_3d"].shape[0] for r in det.simple_test(pts, metas, img=img, **kw))
    print(json.dumps(dict(what="simple_test", input="images", batch=B, ms=round(ms, 3), boxes=n)))


if __name__ == "__main__":
    main()
