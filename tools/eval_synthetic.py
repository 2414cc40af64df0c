#!/usr/bin/env python
"""Score detections on the synthetic scenes with the device evaluator (isfusion_amd.evaluation).

  python tools/eval_synthetic.py [--batch 2] [--points 60000] [--trained N] [--camera]
      builds ISFusionPtsPath (or ISFusionDetector with --camera) with seeded weights, runs the device half of
      simple_test (forward_pts + decode_and_nms), feeds NuScenesDetectionEval with synthetic.scene_boxes and prints
      detail().  --trained N runs N detection-loss steps first and prints the metrics before and after.
  python tools/eval_synthetic.py --rows 6019 [--preds 200] [--boxes 30]
      no model: seeded synthetic rows of that size (a nuScenes-val-sized problem), for the timing alone.

Both print the time of compute() beside the time of the float64 host restatement (tests/eval_common.py) on the same rows
and the largest difference between the two.  A helper, not a judged line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def synthetic_rows(seed, S, P, G):
    """S samples of P predictions and G boxes, vectorised: the first ~85 % of the boxes get a prediction near them (noise
    scale 0.1 .. 2.5 m) with the higher scores, the rest of the P rows is clutter; distinct scores"""
    import eval_common as EC
    rng = np.random.default_rng(seed)
    C = len(EC.CLASSES)

    def boxes(n):
        b = np.empty((S, n, 9), np.float32)
        b[..., :2] = rng.uniform(-48, 48, (S, n, 2))
        b[..., 2] = -1.0
        b[..., 3:6] = rng.uniform(0.4, 5.0, (S, n, 3))
        b[..., 6] = rng.uniform(-np.pi, np.pi, (S, n))
        b[..., 7:9] = rng.normal(0, 1.0, (S, n, 2)) * (rng.random((S, n, 1)) < 0.6)
        return b
    gb, gl = boxes(G), rng.integers(0, C, (S, G)).astype(np.int32)
    pb, pl = boxes(P), rng.integers(0, C, (S, P)).astype(np.int32)
    n = min(G, P)
    near = rng.random((S, n)) < 0.85
    noisy = gb[:, :n].copy()
    noisy[..., :2] += (rng.normal(0, 1, (S, n, 2)) * rng.choice([0.1, 0.4, 1.0, 2.5], (S, n, 1))).astype(np.float32)
    noisy[..., 3:6] *= rng.uniform(0.8, 1.25, (S, n, 3)).astype(np.float32)
    noisy[..., 6] += rng.normal(0, 0.3, (S, n)).astype(np.float32)
    pb[:, :n] = np.where(near[..., None], noisy, pb[:, :n])
    pl[:, :n] = np.where(near, gl[:, :n], pl[:, :n])
    quality = rng.random((S, P))
    quality[:, :n] += 0.7 * near
    scores = np.empty((S, P), np.float32)
    ranked = np.sort(EC.distinct_scores(rng, S * P).reshape(S, P), axis=1)[:, ::-1]
    np.put_along_axis(scores, np.argsort(-quality, axis=1), ranked, axis=1)
    ga = rng.integers(-1, 8, (S, G)).astype(np.int32)
    gn = rng.integers(0, 12, (S, G)).astype(np.int32)
    valid = rng.random((S, P)) < 0.95
    return [EC.make_sample(pb[s], scores[s], pl[s], gb[s], gl[s], valid=valid[s], gt_attrs=ga[s], gt_num_pts=gn[s])
            for s in range(S)]


def report(ev, samples, what, repeats=30):
    """compute() (timed, device) beside the host restatement (timed) on the same rows"""
    import eval_common as EC
    ev.compute()                                            # warm: library, workspace
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):                                # host clock around a call that ends in its one sync
        t0 = time.perf_counter()
        got = ev.compute()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    t0 = time.perf_counter()
    ref = EC.evaluate(samples)
    host_s = time.perf_counter() - t0
    err, where = EC.max_metric_error(got, ref["metrics"])
    masks_equal = bool(np.array_equal(ev.tp_masks().cpu().numpy(), np.concatenate(ref["tp_masks"])))
    print(json.dumps({"what": what, "samples": len(samples), "prediction_rows": int(sum(len(s["labels"]) for s in samples)),
                      "gt_boxes": int(sum(len(s["gt_labels"]) for s in samples)), "compute_ms_median": round(times[len(times) // 2], 3),
                      "compute_ms_min_max": [round(times[0], 3), round(times[-1], 3)], "compute_calls": repeats,
                      "host_restatement_s": round(host_s, 3), "max_abs_metric_diff": err, "at": where,
                      "tp_masks_equal": masks_equal, "mAP": got["mean_ap"], "NDS": got["nd_score"]}))
    return got


def rows_mode(a, dev):
    import eval_common as EC
    from isfusion_amd import evaluation
    t0 = time.perf_counter()
    samples = synthetic_rows(a.seed, a.rows, a.preds, a.boxes)
    print(f"generated {a.rows} x {a.preds} predictions, {a.boxes} boxes each in {time.perf_counter() - t0:.1f} s")
    ev = evaluation.NuScenesDetectionEval(EC.CLASSES, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    EC.feed(ev, samples, batch=a.update_batch, device=dev)
    torch.cuda.synchronize()
    print(f"{-(-a.rows // a.update_batch)} update() calls: {(time.perf_counter() - t0) * 1e3:.1f} ms (with the uploads)")
    report(ev, samples, "synthetic rows")
    for k, v in ev.detail().items():
        if k.endswith(("NDS", "mAP", "mATE", "mASE", "mAOE", "mAVE", "mAAE")):
            print(f"  {k}: {v}")


def model_mode(a, dev):
    import eval_common as EC
    from isfusion_amd import evaluation, head_loss, synthetic
    from isfusion_amd.detector import ISFusionDetector, ISFusionPtsPath
    from isfusion_amd.fusion_modules import seeded_state_dict
    if a.camera:
        net = ISFusionDetector(
            img_backbone=dict(type="SwinTransformer", embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24],
                              window_size=7, mlp_ratio=4, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0,
                              drop_path_rate=0.2, patch_norm=True, out_indices=[1, 2, 3], with_cp=False,
                              convert_weights=False),
            img_neck=dict(type="GeneralizedLSSFPN", in_channels=[192, 384, 768], out_channels=256, start_level=0,
                          num_outs=3), detach=True)
    else:
        net = ISFusionPtsPath()
    net._lidar.randomize_weights_(0).randomize_bn_(1)
    for mod, seed in ((net.fusion_encoder, 100), (net.pts_backbone, 200), (net.pts_neck, 250)):
        mod.load_state_dict(seeded_state_dict(mod, seed))
    if net.pts_bbox_head.train_cfg is None:
        net.pts_bbox_head.train_cfg = dict(head_loss.SHIPPED_TRAIN_CFG)
    net = net.to(dev)
    pts = [torch.from_numpy(synthetic.lidar_sweeps(9000 + i, a.points)).to(dev) for i in range(a.batch)]
    scenes = [synthetic.scene_boxes(9000 + i) for i in range(a.batch)]
    gt = ([torch.from_numpy(b).to(dev) for b, _ in scenes], [torch.from_numpy(l).to(dev) for _, l in scenes])
    inp = synthetic.fusion_inputs(7, a.batch)
    kw = dict(lidar2img=torch.from_numpy(inp["lidar2img"]), img_aug_matrix=torch.from_numpy(inp["img_aug_matrix"]),
              lidar_aug_matrix=torch.from_numpy(inp["lidar_aug_matrix"]))
    metas = [dict(input_shape=inp["input_shape"]) for _ in range(a.batch)]
    if a.camera:
        h, w = inp["input_shape"]
        img = torch.randn(a.batch, 6, 3, h, w, generator=torch.Generator().manual_seed(70)).to(dev)
    else:
        img = tuple(torch.from_numpy(x).to(dev) for x in inp["img_feats"])
    ev = evaluation.NuScenesDetectionEval(EC.CLASSES, device=dev)

    def score(what):
        net.eval()
        ev.reset()
        with torch.no_grad():
            feats = net.extract_img_feat(img, metas) if a.camera else img
            outs = net.forward_pts(pts, feats, metas, **kw)
            boxes, scores, labels, counts, keep = net.pts_bbox_head.decode_and_nms(outs)
        ev.update(boxes, scores, labels, keep if keep is not None else counts, gt[0], gt[1])    # no host sync
        hv = keep.cpu().numpy() if keep is not None else \
            np.arange(boxes.shape[1])[None, :] < counts.cpu().numpy()[:, None]
        hb, hs, hl = boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy()
        samples = [EC.make_sample(hb[i], hs[i], hl[i], scenes[i][0], scenes[i][1], valid=hv[i]) for i in range(a.batch)]
        report(ev, samples, what)
        for k, v in ev.detail().items():
            print(f"  {k}: {v}")

    score("seeded weights")
    if a.trained > 0:
        net.train()
        opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=a.lr, momentum=0.9)
        for step in range(a.trained):
            if a.camera:
                ld = net.forward_train(points=pts, img_metas=metas, gt_bboxes_3d=gt[0], gt_labels_3d=gt[1], img=img, **kw)
            else:
                ld = net.forward_train(pts, img, metas, gt[0], gt[1], **kw)
            loss = sum(v.float() for k, v in ld.items() if k != "matched_ious")
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            print(f"step {step}: loss {float(loss.detach()):.5f}")
        score(f"after {a.trained} detection-loss steps")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--trained", type=int, default=0, help="detection-loss steps to run before the second scoring")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--camera", action="store_true", help="the whole detector (camera branch on HIP) instead of the points path")
    ap.add_argument("--rows", type=int, default=0, help="no model: this many samples of seeded synthetic rows")
    ap.add_argument("--preds", type=int, default=200)
    ap.add_argument("--boxes", type=int, default=30)
    ap.add_argument("--update-batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=2019)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.rows > 0:
        rows_mode(a, dev)
    else:
        model_mode(a, dev)


if __name__ == "__main__":
    main()
