"""Time the GT-paste inside the two batch loaders (isf_assemble_points_paste, isf_image_paste) on one GPU, at the size
a training batch has: B = 4 samples x 300 k points (key frame + 9 sweeps) with 30 sampled boxes per sample, and
6 x 900 x 1600 images with 30 pasted patches (plus the real-GT mix-backs) per sample.  Per repeat, alternating:
  * points   MultiSweepPointLoader(frames) without plans, and with plans (both calls end in their one stream sync:
             wall clock of the whole call, files already in memory)
  * images   MultiViewImageLoader.launch on staged buffers (device events: isf_image_prepass alone, and
             isf_image_paste + isf_image_prepass), and stage() + launch() end to end (wall clock, synchronised)
  * numpy    the same paste restated on the host as the reference's dataloader worker runs it, per sample: the
             vectorised plane test over every point and box + concatenation, and the uint8 rectangle operations on
             the decoded arrays (without the reference's PIL round trip of the whole image per object)
The overhead of the paste is the difference between the two loader timings.

    python tools/gt_paste_bench.py [--steps 20] [--warmup 3] [--repeats 3]

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isfusion_amd import gt_paste, synthetic  # noqa: E402
from isfusion_amd import input_pipeline as ip  # noqa: E402

B, VIEWS, SRC_HW, FINAL_DIM = 4, 6, (900, 1600), (384, 1056)
KEY_POINTS, SWEEPS, BOXES, MIXUP = 30000, 9, 30, 0.7
PC_RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]


def make_sample(seed):
    """-> (point frame dict, image result dict, plan) with 30 sampled boxes / patches"""
    rng = np.random.default_rng(seed)
    cloud = synthetic.lidar_sweeps(seed, KEY_POINTS * (SWEEPS + 1))
    per = len(cloud) // (SWEEPS + 1)
    frame = dict(pts_filename=cloud[:per], timestamp=1.0,
                 sweeps=[dict(data_path=cloud[(k + 1) * per:(k + 2) * per], timestamp=1e6 - 5e4 * (k + 1),
                              sensor2lidar_rotation=np.eye(3), sensor2lidar_translation=np.array([0.1 * k, 0.0, 0.0]))
                         for k in range(SWEEPS)])
    imgs = [rng.integers(0, 256, SRC_HW + (3,), dtype=np.uint8) for _ in range(VIEWS)]
    boxes = np.zeros((BOXES, 9), np.float32)
    boxes[:, :2] = rng.uniform(-45, 45, (BOXES, 2))
    boxes[:, 2] = -1.8
    boxes[:, 3:6] = rng.uniform([1.5, 1.5, 1.0], [8.0, 3.0, 3.0], (BOXES, 3))
    boxes[:, 6] = rng.uniform(-np.pi, np.pi, BOXES)
    objects, ops = [], []
    for k in range(BOXES):
        pts = np.zeros((60, 5), np.float32)
        pts[:, :3] = rng.uniform(-0.4, 0.4, (60, 3)) * boxes[k, 3:6]
        h, w = int(rng.integers(40, 200)), int(rng.integers(60, 300))
        y0, x0 = int(rng.integers(0, SRC_HW[0] - h)), int(rng.integers(0, SRC_HW[1] - w))
        objects.append(dict(points=pts, translation=boxes[k, :3].copy(),
                            patch=rng.integers(0, 256, (h, w, 3), dtype=np.uint8), name="car", index=k))
        if k % 5 == 0:                                    # a real ground-truth box mixed back in front of it
            ops.append(dict(view=k % VIEWS, kind="mix", rows=(y0, min(y0 + 120, SRC_HW[0])), cols=(x0, x0 + 60)))
        mh, mw = int(0.05 * h), int(0.05 * w)
        ops.append(dict(view=k % VIEWS, kind="patch", rows=(y0, y0 + h), cols=(x0, x0 + w), object=k,
                        mask_rows=(y0 + mh, y0 + h - mh), mask_cols=(x0 + mw, x0 + w - mw)))
    plan = gt_paste.GTPastePlan(objects=objects, planes=gt_paste.box_planes(boxes).astype(np.float32), image_ops=ops,
                                mixup=MIXUP, sample_2d=True)
    return frame, dict(img=imgs), plan


def numpy_points(frame, plan):
    """ObjectSampleV2's point side on the host, vectorised (the reference loops in numba on one core)"""
    pts = np.concatenate([frame["pts_filename"]] + [s["data_path"] for s in frame["sweeps"]])
    planes = plan.planes
    inside = np.zeros(len(pts), bool)
    for q in planes:
        sign = pts[:, 0:1] * q[None, :, 0] + pts[:, 1:2] * q[None, :, 1] + pts[:, 2:3] * q[None, :, 2] + q[None, :, 3]
        inside |= (sign < 0).all(1)
    objs = [o["points"] + np.concatenate([o["translation"], [0, 0]]).astype(np.float32) for o in plan.objects]
    return np.concatenate(objs + [pts[~inside]])


def numpy_images(result, plan):
    imgs = [im.copy() for im in result["img"]]
    for op in plan.image_ops:
        (r0, r1), (c0, c1) = op["rows"], op["cols"]
        im = imgs[op["view"]]
        if op["kind"] == "mix":
            im[r0:r1, c0:c1] = MIXUP * result["img"][op["view"]][r0:r1, c0:c1] + (1 - MIXUP) * im[r0:r1, c0:c1]
        else:
            mask = np.zeros((r1 - r0, c1 - c0))
            mask[op["mask_rows"][0] - r0:op["mask_rows"][1] - r0, op["mask_cols"][0] - c0:op["mask_cols"][1] - c0] = 1.0
            patch = plan.objects[op["object"]]["patch"][:r1 - r0, :c1 - c0]
            im[r0:r1, c0:c1] = (im[r0:r1, c0:c1].astype(np.float32) * (1 - mask * MIXUP)[..., None]).astype(np.uint8)
            im[r0:r1, c0:c1] += (MIXUP * patch.astype(np.float32) * mask[..., None]).astype(np.uint8)
    return imgs


def wall(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    samples = [make_sample(100 + b) for b in range(B)]
    frames, results, plans = [s[0] for s in samples], [s[1] for s in samples], [s[2] for s in samples]
    points = ip.MultiSweepPointLoader(sweeps_num=10, test_mode=True, point_cloud_range=PC_RANGE, device=dev)
    images = ip.MultiViewImageLoader(final_dim=FINAL_DIM, resize_lim=[0.57, 0.825], bot_pct_lim=[0.0, 0.0],
                                     rot_lim=[-5.4, 5.4], rand_flip=True, is_train=True, mean=[0.485, 0.456, 0.406],
                                     std=[0.229, 0.224, 0.225], device=dev)
    np.random.seed(0)
    draws = [[images.sample_augmentation((SRC_HW[1], SRC_HW[0])) for _ in range(VIEWS)] for _ in range(B)]
    aug = [ip.draw_train_aug() for _ in range(B)]
    out = torch.empty((B * VIEWS, 3) + FINAL_DIM, dtype=torch.float32, device=dev)
    removed = sum(p.shape[0] for p in points(frames, aug=aug)) - sum(p.shape[0] for p in points(frames, aug=aug,
                                                                                                 paste=plans))

    def device_ms(with_paste):
        staged = images.stage(results, aug=draws, paste=plans if with_paste else None)
        backup = staged["raw"].clone()
        spec = staged.get("paste")
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        total = 0.0
        for i in range(a.warmup + a.steps):
            staged["raw"].copy_(backup)                   # the paste is in place: every launch starts from the upload
            if spec is not None:
                staged["paste"] = spec
            beg.record()
            images.launch(staged, out)
            end.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                total += beg.elapsed_time(end)
        return total / a.steps

    rec = {k: [] for k in ("points_plain_ms", "points_paste_ms", "image_device_plain_ms", "image_device_paste_ms",
                           "image_loader_plain_ms", "image_loader_paste_ms")}
    for _ in range(a.repeats):
        rec["points_plain_ms"].append(wall(lambda: points(frames, aug=aug), a.steps, a.warmup))
        rec["points_paste_ms"].append(wall(lambda: points(frames, aug=aug, paste=plans), a.steps, a.warmup))
        rec["image_device_plain_ms"].append(device_ms(False))
        rec["image_device_paste_ms"].append(device_ms(True))
        rec["image_loader_plain_ms"].append(wall(lambda: images(results, aug=draws, out=out), a.steps, a.warmup))
        rec["image_loader_paste_ms"].append(wall(lambda: images(results, aug=draws, out=out, paste=plans), a.steps,
                                                 a.warmup))
    t0 = time.perf_counter()
    for f, p in zip(frames, plans):
        numpy_points(f, p)
    host_points = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    for r, p in zip(results, plans):
        numpy_images(r, p)
    host_images = (time.perf_counter() - t0) * 1e3
    med = {k: round(float(np.median(v)), 3) for k, v in rec.items()}
    print(json.dumps(dict(batch=B, points_per_sample=KEY_POINTS * (SWEEPS + 1), boxes_per_sample=BOXES,
                          image_ops_per_sample=len(plans[0].image_ops), points_removed=int(removed), **med,
                          spread={k: [round(min(v), 3), round(max(v), 3)] for k, v in rec.items()},
                          points_paste_overhead_ms=round(med["points_paste_ms"] - med["points_plain_ms"], 3),
                          image_device_paste_overhead_ms=round(med["image_device_paste_ms"]
                                                               - med["image_device_plain_ms"], 3),
                          image_loader_paste_overhead_ms=round(med["image_loader_paste_ms"]
                                                               - med["image_loader_plain_ms"], 3),
                          numpy_points_ms=round(host_points, 1), numpy_images_ms=round(host_images, 1))))


if __name__ == "__main__":
    main()
