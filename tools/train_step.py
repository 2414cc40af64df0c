"""Data-parallel training steps of the point-cloud path under torchrun (BASELINE configs[3] shape: B frames per GPU, RCCL
all-reduce over xGMI on the GRADIENTS only -- the forward has no collective):

    python tools/train_step.py --gpus N [--batch 2] [--points 60000] [--steps 3] [--bf16] [--autocast]
                               [--optimizer sgd|config] [--max-iters M] [--gt-paste] [--camera [--camera-backward] [--camera-precision f32|mixed]]
                               [--deterministic]

starts N ranks by itself (isfusion_amd.launch.self_launch: a re-exec under torch.distributed.run on 127.0.0.1; fewer
than N visible GPUs is an error) -- the reference's tools/run-nus.sh:11-13; under a launcher it runs as the rank it is:

    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port 29540 \
        tools/train_step.py --gpus N [...]

One process per GPU; every rank draws its own synthetic frames.  The module is wrapped in DistributedDataParallel
(bucketed gradient all-reduce overlapped with the backward); the path's BatchNorm layers are the config's:
isfusion_amd.norm.NaiveSyncBatchNorm where the reference uses naiveSyncBN (cross-rank statistics, one all_reduce of
[2C] per layer, whenever the world size is > 1), plain BatchNorm (local-shard statistics) elsewhere.  The default loss is a stand-in (feature energy + heat-map mean); --loss detection trains
on the detection head's real losses (ISFusionPtsPath.forward_train: targets, Hungarian assignment and losses on the HIP
kernels) against the synthetic scenes' boxes (synthetic.scene_boxes).  Prints one JSON line per rank 0 with ms per step.
--gt-paste (with --loss detection) puts ObjectSampleV2 in front of every step: a small database built from other
synthetic scenes' boxes, one isfusion_amd.gt_paste plan per frame, and the points through
MultiSweepPointLoader(paste=...) (isf_assemble_points_paste); the step then trains on the pasted points and the
concatenated boxes.  --camera trains the whole ISFusionDetector from images (6 synthetic views per frame in the shape
MultiViewImageLoader hands over, [B, 6, 3, 384, 1056] float32) instead of precomputed camera features: the Swin backbone's
training-mode forward (stochastic depth, no backward: detach=True), the LSS-FPN neck with its backward, then the same
point-cloud path; --loss detection goes through ISFusionDetector.forward_train.  The backbone and the neck's level-0
convs receive no gradient (only the stride-16 map reaches Point-to-Grid), so --camera FREEZES those parameters
(requires_grad False) rather than asking DistributedDataParallel for find_unused_parameters: no per-step graph search,
and the optimizer skips them.  --camera-backward (with --camera) builds the detector with detach=False and
camera_backward = True instead: the backbone's backward runs (swin.py, isf_swin_train.hip) and only the norm of its
first output map and the neck's level-0 convs stay frozen.  --camera-precision mixed (with --camera) runs the backbone in its
mixed-precision training mode (ISFusionDetector.camera_precision).  --deterministic runs every step under isfusion_amd.set_deterministic(True) (exact,
order-independent accumulation in the four scattering kernels; any --loss / --camera / --optimizer / --gt-paste): the steps
are then bit-identical run to run.  With more than one rank the mode also covers the sums that cross ranks
(isfusion_amd.collectives): the forward runs under ddp.no_sync() and exact_all_reduce_gradients sums the local gradients
in 64-bit fixed point (an integer all-reduce), the naiveSyncBN statistics go through the exact all_reduce_sum_ -- losses,
gradients and updated parameters then depend only on the SET of per-rank inputs and seeds, not on the backend, the
collective's algorithm or the order of the ranks.  --data-order i,j,k deals the data differently: rank r takes the frames,
scenes, images and seeds rank order[r] takes by default.  A deterministic run's JSON line carries `param_digest`, the sha256
of rank 0's parameters and naiveSyncBN buffers after the last step (a plain BatchNorm's running statistics are one
rank's own and stay out): equal for every --data-order and every --backend (`replicas_agree`: every rank's digest is rank
0's).  A deterministic run also seeds torch's, numpy's and Python's generators -- one seed while the model is built, one per
share of the data for the steps (attention dropout, region noise) -- so that it repeats from its command line.  The mode makes no claim about a different
NUMBER of ranks.  Also runs on a single GPU without torchrun (world size 1)."""
import argparse
import contextlib
import json
import os
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# the training recipe of configs/isfusion/isfusion_0075voxel.py:398-413 (tests/golden/isfusion_0075voxel_train.txt)
RECIPE = dict(optimizer=dict(type="AdamW", lr=0.0001, weight_decay=0.01,
                             paramwise_cfg=dict(custom_keys={"img_backbone": dict(lr_mult=0.1)})),
              optimizer_config=dict(grad_clip=dict(max_norm=0.01, norm_type=2)),
              lr_config=dict(policy="cyclic", target_ratio=(10, 0.0001), cyclic_times=1, step_ratio_up=0.4),
              momentum_config=dict(policy="cyclic", target_ratio=(0.8947368421052632, 1), cyclic_times=1,
                                   step_ratio_up=0.4))


def gt_paste_database(first_seed, scenes=4, points_per_object=24):
    """A GT-paste database from the boxes of `scenes` synthetic scenes no rank trains on: every box becomes an entry
    whose points (float32 [n, 5], centred on the box as the database files are) fill it uniformly."""
    import numpy as np
    from isfusion_amd import synthetic
    rng = np.random.default_rng(first_seed)
    names, db = ("car", "truck"), dict(car=[], truck=[])
    for seed in range(first_seed, first_seed + scenes):
        for box, label in zip(*synthetic.scene_boxes(seed)):
            pts = np.zeros((points_per_object, 5), np.float32)
            pts[:, :3] = rng.uniform(-0.45, 0.45, (points_per_object, 3)) * box[3:6]
            pts[:, 2] += box[5] * 0.5
            pts[:, 3] = rng.integers(0, 256, points_per_object)
            db[names[label]].append(dict(name=names[label], path=pts, box3d_lidar=box, num_points_in_gt=points_per_object,
                                         box2d_camera=np.zeros(5, np.float32), difficulty=0))
    return db


def parse_data_order(text, world):
    """--data-order 'i,j,k' -> [i, j, k]: rank r takes what rank order[r] takes by default.  Empty: the identity.  Anything
    but a permutation of range(world) is an error."""
    if not text:
        return list(range(world))
    try:
        order = [int(v) for v in text.split(",")]
    except ValueError:
        raise ValueError(f"--data-order {text!r}: expected comma-separated rank numbers") from None
    if sorted(order) != list(range(world)):
        raise ValueError(f"--data-order {text!r} is not a permutation of the {world} ranks")
    return order


def seed_everything(seed):
    """torch's, numpy's and Python's global generators: initial weights that are not loaded from a seeded state dict, the
    seeds of the attention dropout, the region noise"""
    import random
    import numpy as np
    torch.manual_seed(seed)
    np.random.seed(seed % 2 ** 32)
    random.seed(seed)


def param_digest(module):
    """sha256 over the parameters and the cross-rank buffers of `module`, in state-dict order: every parameter, and the
    buffers of the naiveSyncBN layers (statistics of ALL ranks' rows).  The running statistics of a plain BatchNorm are
    one rank's own -- they follow the data that rank drew, by design -- and are left out."""
    import hashlib
    from isfusion_amd.norm import NaiveSyncBatchNorm1d, NaiveSyncBatchNorm2d
    h = hashlib.sha256()
    for name, p in module.named_parameters():
        h.update(name.encode())
        h.update(p.detach().cpu().numpy().tobytes())
    for mname, mod in module.named_modules():
        if isinstance(mod, (NaiveSyncBatchNorm1d, NaiveSyncBatchNorm2d)):
            for name, b in mod.named_buffers(recurse=False):
                h.update(f"{mname}.{name}".encode())
                h.update(b.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=0, help="ranks to start (0 = whatever the launcher started, else 1)")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--bf16", action="store_true", help="camera features in bfloat16 (the reference's autocast dtype)")
    ap.add_argument("--autocast", action="store_true",
                    help="run forward + loss under torch.autocast(bfloat16): stock convs / linears in bf16, the HIP "
                         "autograd Functions cast their inputs to fp32")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl = RCCL over xGMI (the real thing); gloo with --shared-device = a 1-GPU REHEARSAL of the "
                         "multi-rank step (DDP's bucketed all-reduce and the sync-BN exchange go through gloo)")
    ap.add_argument("--shared-device", action="store_true",
                    help="every rank uses cuda:0 (1-GPU box): proves that several processes of libisf_hip.so train side "
                         "by side; with --backend gloo")
    ap.add_argument("--stock-dense", action="store_true",
                    help="the dense 3x3 conv + BatchNorm stacks on the stock modules (MIOpen) instead of dense_train.py (A/B)")
    ap.add_argument("--loss", default="standin", choices=["standin", "detection"],
                    help="standin: feature energy + heat-map mean (the neck output only); detection: the head's "
                         "forward_train and TransFusionHeadV2.loss on the synthetic scenes' GT boxes")
    ap.add_argument("--optimizer", default="sgd", choices=["sgd", "config"],
                    help="sgd: SGD(lr 1e-4, momentum 0.9) as before; config: the reference's recipe (isfusion_amd.optim."
                         "TrainingRecipe: mmcv per-parameter groups, fused AdamW + grad clip 0.01, cyclic lr / momentum)")
    ap.add_argument("--max-iters", type=int, default=0,
                    help="iterations the cyclic schedules span with --optimizer config (0 = --steps + 1)")
    ap.add_argument("--gt-paste", action="store_true",
                    help="ObjectSampleV2 in front of every step (needs --loss detection): a synthetic database, one "
                         "GT-paste plan per frame, points through isf_assemble_points_paste")
    ap.add_argument("--camera", action="store_true",
                    help="train ISFusionDetector from images (Swin forward_train + LSS-FPN forward_train / backward) instead "
                         "of precomputed camera features; the parameters that get no gradient -- img_backbone.* and the "
                         "neck's level-0 convs -- are frozen (requires_grad False), not left to find_unused_parameters")
    ap.add_argument("--camera-backward", action="store_true",
                    help="with --camera: detach=False and ISFusionDetector.camera_backward = True -- the Swin backbone's "
                         "backward runs too (the reference class's default; the shipped optimizer's lr_mult 0.1 group)")
    ap.add_argument("--camera-precision", default="f32", choices=["f32", "mixed"],
                    help="with --camera: ISFusionDetector.camera_precision -- mixed: the Swin backbone's mixed-precision "
                         "training mode (f16 products, fp32 master weights and gradients)")
    ap.add_argument("--head-cross-dropout", action="store_true",
                    help="with --loss detection: TransFusionHeadV2.cross_attention_dropout = True -- the decoder layer's "
                         "dropout (p = 0.1) on the probabilities of the head's 200 x 32400 cross-attention too")
    ap.add_argument("--deterministic", action="store_true",
                    help="isfusion_amd.set_deterministic(True): the isf_*_det entries (fixed-point accumulation) in "
                         "DynamicScatter, Point-to-Grid backward and both MSDA backwards")
    ap.add_argument("--data-order", default="",
                    help="i,j,k: rank r takes the frames, scenes, images and seeds that rank order[r] takes by default "
                         "(the identity); with --deterministic the step's result does not depend on it")
    a = ap.parse_args()
    if a.camera_backward and not a.camera:
        ap.error("--camera-backward switches the camera branch's backward on: it needs --camera")
    if a.camera_precision != "f32" and not a.camera:
        ap.error("--camera-precision sets the camera backbone's mode: it needs --camera")
    if a.head_cross_dropout and a.loss != "detection":
        ap.error("--head-cross-dropout trains the detection head: it needs --loss detection")
    if a.gt_paste and a.loss != "detection":
        ap.error("--gt-paste pastes ground truth: it needs --loss detection")
    import isfusion_amd
    from isfusion_amd import launch, synthetic
    isfusion_amd.set_deterministic(a.deterministic)
    if a.stock_dense:
        from isfusion_amd import dense_train
        dense_train.ENABLED = False
    if a.gpus > 0:
        launch.self_launch(a.gpus, a.backend)
    from isfusion_amd.detector import ISFusionPtsPath
    from isfusion_amd.fusion_modules import seeded_state_dict
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = 0 if a.shared_device else int(os.environ.get("LOCAL_RANK", "0"))
    try:
        src = parse_data_order(a.data_order, world)[rank]           # whose share of the data this rank takes
    except ValueError as e:
        ap.error(str(e))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29540")
    dist.init_process_group(a.backend, rank=rank, world_size=world)  # "nccl" IS RCCL on ROCm
    if a.deterministic:
        seed_everything(4242)        # a deterministic run repeats from its command line: the same model on every rank ...
    if a.camera:
        from isfusion_amd.detector import ISFusionDetector
        # img_backbone / img_neck / detach of configs/isfusion/isfusion_0075voxel.py:17-45
        net = ISFusionDetector(
            img_backbone=dict(type="SwinTransformer", embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24],
                              window_size=7, mlp_ratio=4, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0,
                              drop_path_rate=0.2, patch_norm=True, out_indices=[1, 2, 3], with_cp=False,
                              convert_weights=False),
            img_neck=dict(type="GeneralizedLSSFPN", in_channels=[192, 384, 768], out_channels=256, start_level=0,
                          num_outs=3), detach=not a.camera_backward).train()
        net.camera_backward = a.camera_backward
        net.camera_precision = a.camera_precision
        g = torch.Generator().manual_seed(4100)
        with torch.no_grad():                                        # O(1) activations through the 12 blocks
            for name, p in list(net.img_backbone.named_parameters()) + list(net.img_neck.named_parameters()):
                if p.dim() > 1 and not name.endswith("relative_position_bias_table"):
                    p.copy_(torch.randn(p.shape, generator=g) * (p[0].numel() ** -0.5))
        # --camera-backward: the backbone trains too; only the norm of its first output map stays without a gradient
        no_grad = ("img_backbone.norm1." if a.camera_backward else "img_backbone.", "img_neck.lateral_convs.0.",
                   "img_neck.fpn_convs.0.")
        for name, p in net.named_parameters():
            if name.startswith(no_grad):
                p.requires_grad_(False)                              # no gradient reaches them (module docstring)
    else:
        net = ISFusionPtsPath().train()
    net._lidar.randomize_weights_(0).randomize_bn_(1)
    for mod, seed in ((net.fusion_encoder, 100), (net.pts_backbone, 200), (net.pts_neck, 250)):
        mod.load_state_dict(seeded_state_dict(mod, seed))
    detection = a.loss == "detection"
    if detection:
        from isfusion_amd import head_loss
        if net.pts_bbox_head.train_cfg is None:
            net.pts_bbox_head.train_cfg = dict(head_loss.SHIPPED_TRAIN_CFG)
        net.pts_bbox_head.cross_attention_dropout = a.head_cross_dropout
    else:
        for p in net.pts_bbox_head.parameters():
            p.requires_grad_(False)                                  # the stand-in loss does not reach the head
    net = net.to(dev)

    class Wrap(torch.nn.Module):                                     # DDP hooks forward(); the path's entry is a method
        def __init__(self, m):
            super().__init__()
            self.m = m

        def forward(self, pts, img, metas, kw, gt=None):
            if a.camera and gt is not None:
                return self.m.forward_train(points=pts, img_metas=metas, gt_bboxes_3d=gt[0], gt_labels_3d=gt[1],
                                            img=img, **kw)
            if a.camera:
                img = self.m.extract_img_feat(img, metas)
            if gt is not None:
                return self.m.forward_train(pts, img, metas, gt[0], gt[1], **kw)
            return self.m.forward_train_pts(pts, img, metas, **kw)

    # gradient_as_bucket_view: the gradients ARE views of the all-reduce buckets -- no per-parameter copy into a bucket
    # after the backward pass (~300 copy launches per step); every parameter that requires a gradient gets one in the
    # step, so no unused-parameter search either
    ddp = torch.nn.parallel.DistributedDataParallel(Wrap(net), device_ids=[local], gradient_as_bucket_view=True)
    if a.deterministic:
        seed_everything(4300 + src)  # ... and the draws of the steps belong to the share of the data, not to the rank
    recipe = None
    if a.optimizer == "config":
        from isfusion_amd.optim import TrainingRecipe
        recipe = TrainingRecipe.from_config(RECIPE, net, a.max_iters or a.steps + 1)
        opt = recipe.optimizer
    else:
        opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-4, momentum=0.9)
    pts = [torch.from_numpy(synthetic.lidar_sweeps(9000 + 100 * src + i, a.points)).to(dev) for i in range(a.batch)]
    gt = None
    if detection:
        scenes = [synthetic.scene_boxes(9000 + 100 * src + i) for i in range(a.batch)]
        gt = ([torch.from_numpy(b).to(dev) for b, _ in scenes], [torch.from_numpy(l).to(dev) for _, l in scenes])
    paste = None
    if a.gt_paste:
        import numpy as np
        from isfusion_amd.gt_paste import GTPasteSampler
        from isfusion_amd.input_pipeline import MultiSweepPointLoader
        np.random.seed(1234 + src)
        # the scenes hold ~38 boxes each, so the per-class ceilings sit above that: a dozen candidates per frame
        sampler = GTPasteSampler(db_infos=gt_paste_database(9900), rate=1.0, classes=["car", "truck"],
                                 sample_groups=dict(car=40, truck=20), sample_2d=False)
        loader = MultiSweepPointLoader(test_mode=True, device=dev)
        frames = [dict(pts_filename=p.cpu().numpy(), timestamp=0.0, sweeps=[]) for p in pts]

        def paste():
            results = [dict(gt_bboxes_3d=b, gt_labels_3d=l) for b, l in scenes]
            plans = [sampler.sample(r) for r in results]
            return (loader(frames, paste=plans), ([torch.from_numpy(r["gt_bboxes_3d"]).to(dev) for r in results],
                                                  [torch.from_numpy(r["gt_labels_3d"]).to(dev) for r in results]),
                    sum(len(p.objects) for p in plans if p is not None))
    inp = synthetic.fusion_inputs(7 + src, a.batch)
    if a.camera:
        h, w = inp["input_shape"]
        img = torch.randn(a.batch, 6, 3, h, w, generator=torch.Generator().manual_seed(70 + src)).to(dev)
    else:
        img = tuple(torch.from_numpy(x).to(dev).to(torch.bfloat16 if a.bf16 else torch.float32) for x in inp["img_feats"])
    kw = dict(lidar2img=torch.from_numpy(inp["lidar2img"]), img_aug_matrix=torch.from_numpy(inp["img_aug_matrix"]),
              lidar_aug_matrix=torch.from_numpy(inp["lidar_aug_matrix"]))
    metas = [dict(input_shape=inp["input_shape"]) for _ in range(a.batch)]
    # deterministic mode across ranks: DDP leaves the gradients local (no_sync) and the exact reduction sums them, the
    # same bits under every backend and every order of the ranks (isfusion_amd.collectives)
    exact = a.deterministic and world > 1
    if exact:
        from isfusion_amd.collectives import exact_all_reduce_gradients
        reduced = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    losses, norms, pasted, t0 = [], [], [], None
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 2)]   # per-step GPU time stamps (no extra sync)
    for step in range(a.steps + 1):
        marks[step].record()
        if step == 1:
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
        if paste is not None:
            pts, gt, count = paste()
            pasted.append(count)
        with ddp.no_sync() if exact else contextlib.nullcontext(), \
                torch.autocast("cuda", dtype=torch.bfloat16, enabled=a.autocast):
            if detection:
                ld = ddp(pts, img, metas, kw, gt)
                loss = sum(v.float() for k, v in ld.items() if k != "matched_ious")
            else:
                out, hm = ddp(pts, img, metas, kw)
                loss = (out[0].float() ** 2).mean() + hm.float().sigmoid().mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()                                              # bucketed RCCL all-reduce inside ...
        if exact:
            exact_all_reduce_gradients(reduced)                      # ... or local gradients (no_sync) and the exact sum
        if recipe is not None:
            norms.append(float(recipe.step(step)))                  # the device scalar is rewritten by the next step
        else:
            opt.step()
        losses.append(float(loss))
    marks[a.steps + 1].record()
    torch.cuda.synchronize()
    dist.barrier()
    dt = (time.perf_counter() - t0) / max(a.steps, 1)
    per_step = [round(marks[i].elapsed_time(marks[i + 1]), 1) for i in range(a.steps + 1)]   # [0] = the warm-up step
    digest = {}
    if a.deterministic:
        digest["param_digest"] = param_digest(net)
        if world > 1:                                                # the replicas hold the same bits after the last step
            every = [None] * world
            dist.all_gather_object(every, digest["param_digest"])
            digest["replicas_agree"] = len(set(every)) == 1
    if rank == 0:
        print(json.dumps({"world_size": world, "n_gpus": world, "parallelism": f"dp{world}", "rccl": launch.rccl_version(), "backend": a.backend, "shared_device": a.shared_device, "HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"), "batch_per_gpu": a.batch, "points": a.points, "bf16_camera_features": a.bf16, "autocast_bf16": a.autocast, "loss": a.loss, "camera": a.camera, "camera_backward": a.camera_backward, "camera_precision": a.camera_precision, "deterministic": a.deterministic,
                          "head_cross_dropout": a.head_cross_dropout, "ms_per_train_step": round(dt * 1e3, 2), "ms_each_step_gpu_clock": per_step, "losses": [round(v, 5) for v in losses],
                          "optimizer": a.optimizer, **({"grad_norm": [round(n, 6) for n in norms]} if recipe else {}),
                          **({"gt_paste_objects": pasted} if paste is not None else {}),
                          **digest}))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
