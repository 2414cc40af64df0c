"""Time the NMS post-processing and the test-time augmentation on one GPU (device events, after warm-up), on the
seeded synthetic frames of the benchmark (300 k-point sweeps, 6 cameras):
  * TransFusionHeadV2.get_bboxes at B = 2 with nms_type None / 'circle' / 'rotate' (on the head outputs of one forward)
  * ISFusionPtsPath.aug_test with 2 and 4 flip views of one frame against simple_test of that frame
  * the segmented-NMS launch alone (the TTA merge's per-class rotate NMS over 4 x 200 rows)

    python tools/tta_bench.py [--steps 20] [--warmup 3] [--points 300000]

Prints one JSON line per measurement (ms per call, mean over --steps)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isfusion_amd import nms, synthetic  # noqa: E402
from isfusion_amd.detector import ISFusionPtsPath  # noqa: E402
from isfusion_amd.fusion_modules import seeded_state_dict  # noqa: E402
from isfusion_amd.input_pipeline import flip_tta_views  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=300000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    net = ISFusionPtsPath().eval()
    net._lidar.randomize_weights_(0).randomize_bn_(1)
    for name, seed in (("fusion_encoder", 100), ("pts_backbone", 200), ("pts_neck", 250), ("pts_bbox_head", 300)):
        getattr(net, name).load_state_dict(seeded_state_dict(getattr(net, name), seed))
    net = net.to(dev)
    net.freeze()
    head = net.pts_bbox_head
    head.test_cfg = dict(head.test_cfg, **nms.TTA_DEFAULTS)
    B = 2
    pts = [torch.from_numpy(p).to(dev) for p in synthetic.batch(2, B, a.points)]
    inp = synthetic.fusion_inputs(5, B)
    img = tuple(torch.from_numpy(x).to(dev) for x in inp["img_feats"])
    kw = dict(lidar2img=torch.from_numpy(inp["lidar2img"]), img_aug_matrix=torch.from_numpy(inp["img_aug_matrix"]),
              lidar_aug_matrix=torch.from_numpy(inp["lidar_aug_matrix"]))
    metas = [dict(input_shape=inp["input_shape"]) for _ in range(B)]
    with torch.no_grad():
        x = net.pts_neck(net.extract_pts_feat(pts, img, metas, **kw))
        outs = head(x, img, metas)
    base_cfg = dict(head.test_cfg)
    for nms_type in (None, "circle", "rotate"):
        head.test_cfg = dict(base_cfg, nms_type=nms_type)
        ms = timed(lambda: head.get_bboxes(outs, metas), a.steps, a.warmup)
        n = sum(r[0].shape[0] for r in head.get_bboxes(outs, metas))
        print(json.dumps(dict(what="get_bboxes", batch=B, nms_type=nms_type, ms=round(ms, 4), boxes=n)))
    head.test_cfg = base_cfg
    # the TTA merge's NMS launch alone: 4 views x 200 rows, 10 classes
    boxes, scores, labels, counts, _ = head.decode_and_nms(outs)
    rows = torch.cat([boxes.reshape(-1, boxes.shape[-1])] * 2)
    sc = torch.cat([scores.reshape(-1)] * 2)
    valid = torch.arange(boxes.shape[1], device=dev)[None] < counts[:, None].long()
    lab = torch.cat([torch.where(valid, labels, torch.full_like(labels, -1)).reshape(-1)] * 2)
    ms = timed(lambda: nms.segmented_nms(rows, sc, ["rotate"] * 10, [0.2] * 10, rows.shape[0], labels=lab,
                                         task_of_class=list(range(10))), a.steps, a.warmup)
    print(json.dumps(dict(what="segmented_nms", rows=rows.shape[0], segments=10, mode="rotate", ms=round(ms, 4))))
    # aug_test of one frame vs simple_test
    one = dict(lidar2img=kw["lidar2img"][:1], img_aug_matrix=kw["img_aug_matrix"][:1])
    img1 = tuple(f[:6] for f in img)
    m0 = dict(metas[0], lidar_aug_matrix=kw["lidar_aug_matrix"][0].numpy())
    ms = timed(lambda: net.simple_test(pts[:1], [m0], img1, lidar_aug_matrix=kw["lidar_aug_matrix"][:1], **one),
               a.steps, a.warmup)
    print(json.dumps(dict(what="simple_test", views=1, ms=round(ms, 3))))
    for views in (2, 4):
        vp, vm = flip_tta_views(pts[0], m0, pcd_vertical_flip=views == 4)
        ms = timed(lambda: net.aug_test(vp, vm, img1, **one), a.steps, a.warmup)
        n = net.aug_test(vp, vm, img1, **one)[0]["pts_bbox"]["scores_3d"].shape[0]
        print(json.dumps(dict(what="aug_test", views=views, ms=round(ms, 3), boxes=n)))


if __name__ == "__main__":
    main()
