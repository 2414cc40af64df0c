"""TransFusionHeadV2 training targets, Hungarian assignment and losses on the HIP kernels of isf_head_loss.hip
(mmdet3d/models/dense_heads/transfusion_head_v2.py:910-1276, core/bbox/assigners/hungarian_assigner.py:85-156).

Everything runs on the caller's stream with no host sync: the per-sample GT counts are tensor SHAPES (host data), the
number of positives and the average factors stay on the device.  The losses are autograd Functions whose backward is
one launch that scales the gradient their forward kernel already wrote.

Only the shipped configuration types are built (configs/isfusion/isfusion_0075voxel.py:139-163): HungarianAssigner3D
with FocalLossCost / BBoxBEVL1Cost / IoU3DCost, FocalLoss(use_sigmoid), L1Loss and GaussianFocalLoss; any other type
raises NotImplementedError naming it."""
import ctypes

import torch

from . import _lib

# configs/isfusion/isfusion_0075voxel.py:139-163 (voxel_size / grid / range of the shipped 0.075 m model)
SHIPPED_TRAIN_CFG = dict(
    dataset="nuScenes",
    assigner=dict(type="HungarianAssigner3D", iou_calculator=dict(type="BboxOverlaps3D", coordinate="lidar"),
                  cls_cost=dict(type="FocalLossCost", gamma=2, alpha=0.25, weight=0.15),
                  reg_cost=dict(type="BBoxBEVL1Cost", weight=0.25), iou_cost=dict(type="IoU3DCost", weight=0.25)),
    pos_weight=-1, gaussian_overlap=0.1, min_radius=2, grid_size=[1440, 1440, 40], voxel_size=[0.075, 0.075, 0.2],
    out_size_factor=8, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2],
    point_cloud_range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0])
SHIPPED_LOSS_CLS = dict(type="FocalLoss", use_sigmoid=True, gamma=2, alpha=0.25, reduction="mean", loss_weight=1.0)
SHIPPED_LOSS_BBOX = dict(type="L1Loss", reduction="mean", loss_weight=0.25)
SHIPPED_LOSS_HEATMAP = dict(type="GaussianFocalLoss", reduction="mean", loss_weight=1.0)


def _require(cfg, type_name, what):
    t = (cfg or {}).get("type")
    if t != type_name:
        raise NotImplementedError(f"{what} type '{t}' is not built here (only the shipped '{type_name}')")


def check_loss_cfgs(loss_cls, loss_bbox, loss_heatmap):
    _require(loss_cls, "FocalLoss", "loss_cls")
    if not loss_cls.get("use_sigmoid", True):
        raise NotImplementedError("loss_cls FocalLoss(use_sigmoid=False) is not built here")
    _require(loss_bbox, "L1Loss", "loss_bbox")
    _require(loss_heatmap, "GaussianFocalLoss", "loss_heatmap")
    if loss_heatmap.get("alpha", 2.0) != 2.0 or loss_heatmap.get("gamma", 4.0) != 4.0:
        raise NotImplementedError("loss_heatmap: only GaussianFocalLoss(alpha=2, gamma=4) is built here")
    for c in (loss_cls, loss_bbox, loss_heatmap):
        if c.get("reduction", "mean") != "mean":
            raise NotImplementedError(f"{c['type']}: only reduction='mean' is built here")


def check_train_cfg(train_cfg):
    a = train_cfg.get("assigner") or {}
    _require(a, "HungarianAssigner3D", "assigner")
    _require(a.get("cls_cost"), "FocalLossCost", "assigner cls_cost")
    _require(a.get("reg_cost"), "BBoxBEVL1Cost", "assigner reg_cost")
    _require(a.get("iou_cost"), "IoU3DCost", "assigner iou_cost")
    calc = a.get("iou_calculator") or dict(type="BboxOverlaps3D", coordinate="lidar")
    _require(calc, "BboxOverlaps3D", "assigner iou_calculator")
    if calc.get("coordinate", "lidar") != "lidar":
        raise NotImplementedError(f"iou_calculator coordinate '{calc.get('coordinate')}' (only 'lidar' is built)")
    if train_cfg.get("sampler") not in (None, dict(type="PseudoSampler")):
        raise NotImplementedError(f"sampler {train_cfg.get('sampler')} (only PseudoSampler is built)")


# ----------------------------------------------------------------------------------------------------------- GT
def pack_gt(gt_bboxes_3d, gt_labels_3d, device):
    """Per-sample GT ([G, 9] LiDARInstance3DBoxes layout, bottom centre; or objects with such a `.tensor`) -> (boxes
    [sum G, box_ld] fp32, labels [sum G] int64, host offsets (ctypes int array), per-sample counts).  The counts are
    the tensors' shapes: no device read."""
    boxes = [g.tensor if hasattr(g, "tensor") else g for g in gt_bboxes_3d]
    if len(boxes) != len(gt_labels_3d):
        raise ValueError(f"{len(boxes)} GT box sets but {len(gt_labels_3d)} label sets")
    counts = [int(b.shape[0]) for b in boxes]
    for b, lab in zip(boxes, gt_labels_3d):
        if b.dim() != 2 or b.shape[1] < 7 or int(lab.shape[0]) != int(b.shape[0]):
            raise ValueError(f"GT boxes must be [G, >= 7] with G labels, got {tuple(b.shape)} / {tuple(lab.shape)}")
    box_ld = min(int(b.shape[1]) for b in boxes) if boxes else 9
    box_ld = 9 if box_ld >= 9 else 7
    cat = torch.cat([b[:, :box_ld].to(device=device, dtype=torch.float32) for b in boxes]).contiguous()
    labels = torch.cat([lab.to(device=device, dtype=torch.int64).reshape(-1) for lab in gt_labels_3d]).contiguous()
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    return cat, labels, (ctypes.c_int * len(off))(*off), counts, box_ld


def gravity_center(boxes):
    """LiDARInstance3DBoxes.gravity_center (core/bbox/structures/lidar_box3d.py): z + dz / 2, the rest unchanged
    (transfusion_head_v2.py:1082-1084)."""
    out = boxes.clone()
    out[:, 2] = boxes[:, 2] + boxes[:, 5] * 0.5
    return out


# ----------------------------------------------------------------------------------------------------------- targets
def heatmap_targets(cfg, num_classes, boxes, labels, offsets, B):
    """get_targets_single's dense heat-map (:1082-1128) for the batch in one launch -> [B, classes, Y, X]."""
    osf = cfg["out_size_factor"]
    X, Y = cfg["grid_size"][0] // osf, cfg["grid_size"][1] // osf
    heatmap = torch.empty((B, num_classes, Y, X), dtype=torch.float32, device=boxes.device)
    prm = (ctypes.c_float * 7)(cfg["voxel_size"][0], cfg["voxel_size"][1], cfg["point_cloud_range"][0],
                               cfg["point_cloud_range"][1], osf, cfg["gaussian_overlap"], cfg["min_radius"])
    _lib.check(_lib.load().isf_head_heatmap_targets(_lib.ptr(boxes), boxes.shape[1] if boxes.dim() == 2 else 9,
                                                    _lib.ptr(labels), offsets, B, num_classes, Y, X, prm,
                                                    _lib.ptr(heatmap), _lib.stream()), "isf_head_heatmap_targets")
    return heatmap


def assign_cost(pd, cfg, coder, num_proposals, boxes, labels, offsets, counts, box_ld):
    """decode + HungarianAssigner3D cost for every (sample, decoder layer) -> (decoded boxes [B, L*P, 9|7],
    cost [B, L, P, gt_stride], iou [B, L, P, gt_stride], gt_stride)."""
    heat = pd["heatmap"].detach().float().contiguous()
    B, C, LP = heat.shape
    L = LP // num_proposals
    ts = [pd[k].detach().float().contiguous() for k in ("center", "height", "dim", "rot")]
    vel = pd["vel"].detach().float().contiguous() if "vel" in pd else None
    gs = max(max(counts), 1)
    dev = heat.device
    dec = torch.empty((B, LP, 9 if vel is not None else 7), dtype=torch.float32, device=dev)
    cost = torch.empty((B, L, num_proposals, gs), dtype=torch.float32, device=dev)
    iou = torch.empty_like(cost)
    a = cfg["assigner"]
    pcr = cfg["point_cloud_range"]
    prm = (ctypes.c_float * 15)(coder["out_size_factor"] * coder["voxel_size"][0],
                                coder["out_size_factor"] * coder["voxel_size"][1], coder["pc_range"][0],
                                coder["pc_range"][1], *[float(v) for v in pcr[:6]], a["cls_cost"].get("weight", 1.0),
                                a["reg_cost"].get("weight", 1.0), a["iou_cost"].get("weight", 1.0),
                                a["cls_cost"].get("alpha", 0.25), a["cls_cost"].get("gamma", 2.0))
    _lib.check(_lib.load().isf_head_assign_cost(_lib.ptr(heat), *[_lib.ptr(t) for t in ts], _lib.ptr(vel), B, C,
                                                num_proposals, L, _lib.ptr(boxes), box_ld, _lib.ptr(labels), offsets,
                                                gs, prm, _lib.ptr(dec), _lib.ptr(cost), _lib.ptr(iou), _lib.stream()),
               "isf_head_assign_cost")
    return dec, cost, iou, gs


def assign(cost, iou, gs, labels, offsets, B, num_proposals, L):
    """linear_sum_assignment of every (sample, layer) cost on the device -> (assigned_gt_inds [B, L*P] int32,
    assigned labels int64, max_overlaps fp32)."""
    dev = cost.device
    ag = torch.empty((B, L * num_proposals), dtype=torch.int32, device=dev)
    al = torch.empty((B, L * num_proposals), dtype=torch.int64, device=dev)
    mo = torch.empty((B, L * num_proposals), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().isf_head_assign(_lib.ptr(cost), _lib.ptr(iou), gs, _lib.ptr(labels), offsets, B,
                                           num_proposals, L, _lib.ptr(ag), _lib.ptr(al), _lib.ptr(mo), _lib.stream()),
               "isf_head_assign")
    return ag, al, mo


def assemble_targets(assigned, max_overlaps, boxes, box_ld, labels, offsets, num_classes, code_size, coder, pos_weight):
    B, LP = assigned.shape
    dev = assigned.device
    out_labels = torch.empty((B, LP), dtype=torch.int64, device=dev)
    label_weights = torch.empty((B, LP), dtype=torch.float32, device=dev)
    bbox_targets = torch.empty((B, LP, code_size), dtype=torch.float32, device=dev)
    bbox_weights = torch.empty_like(bbox_targets)
    ious = torch.empty((B, LP), dtype=torch.float32, device=dev)
    num_pos = torch.empty((1,), dtype=torch.int32, device=dev)
    stats = torch.empty((2,), dtype=torch.float32, device=dev)
    prm = (ctypes.c_float * 5)(coder["out_size_factor"] * coder["voxel_size"][0],
                               coder["out_size_factor"] * coder["voxel_size"][1], coder["pc_range"][0],
                               coder["pc_range"][1], float(pos_weight))
    _lib.check(_lib.load().isf_head_assemble_targets(_lib.ptr(assigned), _lib.ptr(max_overlaps), _lib.ptr(boxes),
                                                     box_ld, _lib.ptr(labels), offsets, B, LP, num_classes, code_size,
                                                     prm, _lib.ptr(out_labels), _lib.ptr(label_weights),
                                                     _lib.ptr(bbox_targets), _lib.ptr(bbox_weights), _lib.ptr(ious),
                                                     _lib.ptr(num_pos), _lib.ptr(stats), _lib.stream()),
               "isf_head_assemble_targets")
    return out_labels, label_weights, bbox_targets, bbox_weights, ious, num_pos, stats


# ----------------------------------------------------------------------------------------------------------- losses
def _scale_grad(raw, scale, grad_output):
    out = torch.empty_like(raw)
    go = grad_output.detach().float().contiguous()
    _lib.check(_lib.load().isf_head_loss_grad_scale(_lib.ptr(raw), raw.numel(), _lib.ptr(scale), _lib.ptr(go),
                                                    _lib.ptr(out), _lib.stream()), "isf_head_loss_grad_scale")
    return out


class GaussianFocalLossFunction(torch.autograd.Function):
    """GaussianFocalLoss(alpha 2, gamma 4, mean, avg_factor = max(#(target == 1), 1)) of clip_sigmoid(logits)
    (transfusion_head_v2.py:1172-1184); the gradient goes to the logits through the clamp."""

    @staticmethod
    def forward(ctx, logits, target, loss_weight):
        _lib.require_cuda(logits, target)
        x = logits.detach().float().contiguous()
        t = target.detach().float().contiguous()
        if x.shape != t.shape:
            raise ValueError(f"heat-map logits {tuple(x.shape)} vs target {tuple(t.shape)}")
        dev = x.device
        part = torch.empty((512,), dtype=torch.float64, device=dev)
        raw = torch.empty_like(x)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        scale = torch.empty((1,), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().isf_gaussian_focal_loss(_lib.ptr(x), _lib.ptr(t), x.numel(), float(loss_weight),
                                                       _lib.ptr(part), _lib.ptr(raw), _lib.ptr(loss), _lib.ptr(scale),
                                                       _lib.stream()), "isf_gaussian_focal_loss")
        ctx.save_for_backward(raw, scale)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        raw, scale = ctx.saved_tensors
        return _scale_grad(raw, scale, grad_loss), None, None


class SigmoidFocalLossFunction(torch.autograd.Function):
    """FocalLoss(use_sigmoid, gamma, alpha, mean, avg_factor = max(num_pos, 1)) of the proposals' class logits
    [B, classes, L*P], columns [offset, offset + P) (:1212-1226); label == classes is background."""

    @staticmethod
    def forward(ctx, logits, labels, label_weights, num_pos, offset, num_proposals, gamma, alpha, loss_weight):
        _lib.require_cuda(logits)
        x = logits.detach().float().contiguous()
        B, C, LD = x.shape
        raw = torch.zeros_like(x)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        scale = torch.empty((1,), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().isf_sigmoid_focal_loss(_lib.ptr(x), B, C, num_proposals, LD, offset,
                                                      _lib.ptr(labels.contiguous()),
                                                      _lib.ptr(label_weights.float().contiguous()), _lib.ptr(num_pos),
                                                      float(alpha), float(gamma), float(loss_weight), _lib.ptr(raw),
                                                      _lib.ptr(loss), _lib.ptr(scale), _lib.stream()),
                   "isf_sigmoid_focal_loss")
        ctx.save_for_backward(raw, scale)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        raw, scale = ctx.saved_tensors
        return (_scale_grad(raw, scale, grad_loss),) + (None,) * 8


class L1LossFunction(torch.autograd.Function):
    """L1Loss(mean, avg_factor = max(num_pos, 1)) of [center, height, dim, rot, vel] (each [B, k, L*P], columns
    [offset, offset + P)) vs bbox_targets, weighted by bbox_weights * code_weights (:1228-1266)."""

    @staticmethod
    def forward(ctx, center, height, dim, rot, vel, bbox_targets, bbox_weights, code_weights, num_pos, offset,
                num_proposals, loss_weight):
        ts = [t.detach().float().contiguous() for t in (center, height, dim, rot)]
        v = vel.detach().float().contiguous() if vel is not None else None
        B, _, LD = ts[0].shape
        code = 10 if v is not None else 8
        raw = torch.zeros((B, code, LD), dtype=torch.float32, device=ts[0].device)
        loss = torch.empty((), dtype=torch.float32, device=ts[0].device)
        scale = torch.empty((1,), dtype=torch.float32, device=ts[0].device)
        cw = (ctypes.c_float * 10)(*[float(w) for w in list(code_weights)[:code]], *([0.0] * (10 - code)))
        _lib.check(_lib.load().isf_head_l1_loss(*[_lib.ptr(t) for t in ts], _lib.ptr(v), B, num_proposals, LD, offset,
                                                code, _lib.ptr(bbox_targets.contiguous()),
                                                _lib.ptr(bbox_weights.contiguous()), cw, _lib.ptr(num_pos),
                                                float(loss_weight), _lib.ptr(raw), _lib.ptr(loss), _lib.ptr(scale),
                                                _lib.stream()), "isf_head_l1_loss")
        ctx.has_vel = v is not None
        ctx.save_for_backward(raw, scale)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        raw, scale = ctx.saved_tensors
        g = _scale_grad(raw, scale, grad_loss)
        gv = g[:, 8:10] if ctx.has_vel else None
        return (g[:, 0:2], g[:, 2:3], g[:, 3:6], g[:, 6:8], gv) + (None,) * 7


# ----------------------------------------------------------------------------------------------------------- driver
def get_targets(head, gt_bboxes_3d, gt_labels_3d, pd):
    """TransFusionHeadV2.get_targets (:910-960) for the whole batch -> (labels, label_weights, bbox_targets,
    bbox_weights, ious, num_pos, matched_ious, heatmap); num_pos / matched_ious are device scalars (the reference
    returns host numbers, one sync each)."""
    cfg = head.train_cfg
    if cfg is None:
        raise RuntimeError("TransFusionHeadV2.get_targets needs train_cfg (model.train_cfg.pts)")
    dev = pd["heatmap"].device
    _lib.require_cuda(pd["heatmap"])
    B = pd["heatmap"].shape[0]
    if len(gt_bboxes_3d) != B:
        raise ValueError(f"{len(gt_bboxes_3d)} GT sets for a batch of {B}")
    boxes, labels, offsets, counts, box_ld = pack_gt(gt_bboxes_3d, gt_labels_3d, dev)
    P = head.num_proposals
    L = head.num_decoder_layers if head.auxiliary else 1
    coder = head.bbox_coder
    code_size = coder.get("code_size", 10)
    _, cost, iou, gs = assign_cost(pd, cfg, coder, P, boxes, labels, offsets, counts, box_ld)
    assigned, _, mo = assign(cost, iou, gs, labels, offsets, B, P, L)
    lab, lw, bt, bw, ious, num_pos, stats = assemble_targets(assigned, mo, boxes, box_ld, labels, offsets,
                                                             head.num_classes, code_size, coder,
                                                             cfg.get("pos_weight", -1))
    heatmap = heatmap_targets(cfg, head.num_classes, boxes, labels, offsets, B)
    return lab, lw, bt, bw, ious, num_pos[0], stats[1], heatmap


def loss(head, gt_bboxes_3d, gt_labels_3d, preds_dicts, ins_heatmap=None):
    """TransFusionHeadV2.loss (:1143-1276) -> dict(loss_heatmap, [loss_heatmap_ins], layer_-1_loss_cls,
    layer_-1_loss_bbox, matched_ious)."""
    pd = preds_dicts[0][0]
    labels, label_weights, bbox_targets, bbox_weights, _, num_pos, matched_ious, heatmap = get_targets(
        head, gt_bboxes_3d, gt_labels_3d, pd)
    npos = num_pos.reshape(1)
    out = dict()
    out["loss_heatmap"] = GaussianFocalLossFunction.apply(pd["dense_heatmap"], heatmap,
                                                          head.loss_heatmap.get("loss_weight", 1.0))
    if ins_heatmap is not None:
        out["loss_heatmap_ins"] = GaussianFocalLossFunction.apply(ins_heatmap, heatmap,
                                                                  head.loss_heatmap.get("loss_weight", 1.0))
    P = head.num_proposals
    L = head.num_decoder_layers if head.auxiliary else 1
    cw = head.train_cfg.get("code_weights") or [1.0] * head.bbox_coder.get("code_size", 10)
    lc, lb = head.loss_cls, head.loss_bbox
    for i in range(L):
        prefix = "layer_-1" if i == head.num_decoder_layers - 1 or (i == 0 and not head.auxiliary) else f"layer_{i}"
        out[f"{prefix}_loss_cls"] = SigmoidFocalLossFunction.apply(
            pd["heatmap"], labels, label_weights, npos, i * P, P, lc.get("gamma", 2.0), lc.get("alpha", 0.25),
            lc.get("loss_weight", 1.0))
        out[f"{prefix}_loss_bbox"] = L1LossFunction.apply(
            pd["center"], pd["height"], pd["dim"], pd["rot"], pd.get("vel"), bbox_targets, bbox_weights, cw, npos,
            i * P, P, lb.get("loss_weight", 1.0))
    out["matched_ious"] = matched_ious
    return out
