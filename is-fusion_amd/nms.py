"""BEV NMS and the test-time-augmentation merge on the HIP kernels of isf_nms.hip.

Reference interface (mmdet3d/ops/iou3d/iou3d_utils.py, core/post_processing/box3d_nms.py, core/post_processing/
merge_augs.py, core/bbox/transforms.py, core/bbox/structures/utils.py):

    boxes_iou_bev(a [M,5], b [N,5]) -> [M, N]                     rotated BEV IoU of xyxyr boxes
    nms_gpu(boxes [N,5], scores, thresh, pre_maxsize, post_max_size) -> kept indices, in kept order
    nms_normal_gpu(boxes [N,5], scores, thresh) -> kept indices, in kept order
    circle_nms(dets [N,3], thresh, post_max_size=83) -> kept indices, in kept order
    xywhr2xyxyr(boxes [N,5]) -> [N, 5]
    bbox3d_mapping_back(boxes, scale_factor, flip_horizontal, flip_vertical) -> mapped copy
    merge_aug_bboxes_3d(aug_results, img_metas, test_cfg) -> dict(boxes_3d, scores_3d, labels_3d)

plus ``segmented_nms``, the batched entry the detection head and the detector use: many independent segments
(sample x task, or class) in one launch, following device-side counts with no host read.

Everything takes and returns device tensors.  Within a segment boxes are ranked by score, descending, equal scores by
lower input index: the reference's torch.sort / np.argsort are not stable, so its order among equal scores is undefined.
The rotated IoU is computed in fp64 (isf_bev.h), the reference's in fp32.
"""
import ctypes

import torch

from . import _lib

MAX_SEGMENT = 1024      # ISF_NMS_MAX_SEGMENT: rows of one group
MAX_TASKS = 16          # ISF_NMS_MAX_TASKS
MAX_CLASSES = 64        # ISF_NMS_MAX_CLASSES
MAX_VIEWS = 16          # ISF_NMS_MAX_VIEWS
MODES = {"keep": 0, "rotate": 1, "normal": 2, "circle": 3}
BOX_XYXYR, BOX_LIDAR = 0, 1
# the TTA keys of the shipped test_cfg (configs/isfusion/isfusion_0075voxel.py:164-176), used when a test_cfg lacks them
TTA_DEFAULTS = dict(use_rotate_nms=True, nms_thr=0.2, max_num=200)


def xywhr2xyxyr(boxes_xywhr):
    """core/bbox/structures/utils.py:66-84"""
    boxes = torch.zeros_like(boxes_xywhr)
    half_w = boxes_xywhr[:, 2] / 2
    half_h = boxes_xywhr[:, 3] / 2
    boxes[:, 0] = boxes_xywhr[:, 0] - half_w
    boxes[:, 1] = boxes_xywhr[:, 1] - half_h
    boxes[:, 2] = boxes_xywhr[:, 0] + half_w
    boxes[:, 3] = boxes_xywhr[:, 1] + half_h
    boxes[:, 4] = boxes_xywhr[:, 4]
    return boxes


def boxes_iou_bev(boxes_a, boxes_b):
    """iou3d_utils.py:6-23: [M, 5] x [N, 5] xyxyr -> [M, N] float32"""
    _lib.require_cuda(boxes_a, boxes_b)
    a, b = boxes_a.float().contiguous(), boxes_b.float().contiguous()
    assert a.dim() == 2 and a.shape[1] == 5 and b.dim() == 2 and b.shape[1] == 5, (a.shape, b.shape)
    out = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    _lib.check(_lib.load().isf_boxes_iou_bev(_lib.ptr(a), a.shape[0], _lib.ptr(b), b.shape[0], _lib.ptr(out),
                                             _lib.stream()), "isf_boxes_iou_bev")
    return out


def _int_array(vals):
    return (ctypes.c_int * max(len(vals), 1))(*[int(v) for v in vals])


def segmented_nms(boxes, scores, modes, thresholds, group_stride, labels=None, counts=None, task_of_class=None,
                  box_format=BOX_LIDAR, pre_maxsize=None, post_max_size=None):
    """NMS over independent segments in one launch (isf_nms_segmented, include/isf_hip.h).

    boxes [G * group_stride, box_ld] (BOX_LIDAR: x, y, z_bottom, dx, dy, dz, yaw, ...; BOX_XYXYR: x1, y1, x2, y2, r),
    scores [G * group_stride]; group g = its first counts[g] rows (counts: device int32 [G] or None = all).
    labels (int32 [rows] or None = every row task 0) map through task_of_class (a list, -1 = dropped) to the tasks;
    modes / thresholds: one per task ('keep' | 'rotate' | 'normal' | 'circle').  Segment (g, t) = row g * T + t of the
    outputs.  -> keep [rows] bool, keep_index [G * T, group_stride] int32 (absolute rows, kept order), keep_count
    [G * T] int32 -- all on the device, no host sync."""
    _lib.require_cuda(boxes, scores, labels, counts)
    T = len(modes)
    assert T == len(thresholds) and 1 <= T <= MAX_TASKS, (modes, thresholds)
    if group_stride > MAX_SEGMENT:
        raise _lib.IsfError(f"segmented_nms: {group_stride} rows in one segment group; the kernel takes at most "
                            f"{MAX_SEGMENT}")
    dev = boxes.device
    b = boxes.float().contiguous()
    rows = b.shape[0]
    assert group_stride > 0 and rows % group_stride == 0, (rows, group_stride)
    G = rows // group_stride
    s = scores.float().contiguous().view(-1)
    assert s.numel() == rows
    lab = labels.to(torch.int32).contiguous().view(-1) if labels is not None else None
    cnt = counts.to(torch.int32).contiguous() if counts is not None else None
    tasks = list(task_of_class) if task_of_class is not None else []
    assert lab is None or 1 <= len(tasks) <= MAX_CLASSES, "labels need a class -> task table"
    pre = -1 if pre_maxsize is None else int(pre_maxsize)
    post = -1 if post_max_size is None else int(post_max_size)
    keep = torch.empty(rows, dtype=torch.uint8, device=dev)
    keep_index = torch.empty((G * T, group_stride), dtype=torch.int32, device=dev)
    keep_count = torch.empty(G * T, dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws_bytes = lib.isf_nms_workspace_size(G, group_stride, T, pre)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    thr = (ctypes.c_float * T)(*[float(v) for v in thresholds])
    _lib.check(lib.isf_nms_segmented(_lib.ptr(b), b.shape[1], box_format, _lib.ptr(s), _lib.ptr(lab), _lib.ptr(cnt), G,
                                     group_stride, len(tasks), _int_array(tasks), T,
                                     _int_array([MODES[m] for m in modes]), thr, pre, post, _lib.ptr(ws), ws_bytes,
                                     _lib.ptr(keep), _lib.ptr(keep_index), _lib.ptr(keep_count), _lib.stream()),
               "isf_nms_segmented")
    return keep.bool(), keep_index, keep_count


def _single(boxes, scores, mode, thresh, box_format, pre_maxsize=None, post_max_size=None):
    n = boxes.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.long, device=boxes.device)
    _, idx, cnt = segmented_nms(boxes, scores, [mode], [thresh], n, box_format=box_format, pre_maxsize=pre_maxsize,
                                post_max_size=post_max_size)
    return idx[0, :int(cnt.item())].long()           # the reference reads num_out on the host as well


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
    """iou3d_utils.py:26-57: boxes [N, 5] xyxyr; suppressed when the rotated BEV IoU > thresh -> kept indices"""
    return _single(boxes, scores, "rotate", thresh, BOX_XYXYR, pre_maxsize, post_max_size)


def nms_normal_gpu(boxes, scores, thresh):
    """iou3d_utils.py:60-77: boxes [N, 5] xyxyr, axis-aligned IoU of the xyxy corners > thresh -> kept indices"""
    return _single(boxes, scores, "normal", thresh, BOX_XYXYR)


def circle_nms(dets, thresh, post_max_size=83):
    """box3d_nms.py:183-218: dets [N, 3] (x, y, score); suppressed when the SQUARED centre distance <= thresh (the
    reference's semantics: its callers pass a radius as thresh) -> kept indices (a long tensor on the device; the
    reference returns a list)."""
    dets = torch.as_tensor(dets)
    return _single(dets[:, :2], dets[:, 2], "circle", thresh, BOX_XYXYR, None, post_max_size)


def mapping_back_(boxes, num_views, view_stride, scale_factors, flips_horizontal, flips_vertical, counts=None):
    """bbox3d_mapping_back (core/bbox/transforms.py:5-24) in place on rows [v * view_stride, + counts[v]) of a
    contiguous float32 [num_views * view_stride, >= 7] tensor (isf_bbox_mapping_back)."""
    _lib.require_cuda(boxes, counts)
    assert boxes.dtype == torch.float32 and boxes.is_contiguous() and boxes.dim() == 2
    if num_views > MAX_VIEWS:
        raise _lib.IsfError(f"bbox_mapping_back: {num_views} views, at most {MAX_VIEWS}")
    sf = (ctypes.c_float * max(num_views, 1))(*[float(v) for v in scale_factors])
    cnt = counts.to(torch.int32).contiguous() if counts is not None else None
    _lib.check(_lib.load().isf_bbox_mapping_back(_lib.ptr(boxes), boxes.shape[1], num_views, view_stride, _lib.ptr(cnt),
                                                 _int_array(flips_horizontal), _int_array(flips_vertical), sf,
                                                 _lib.stream()), "isf_bbox_mapping_back")
    return boxes


def bbox3d_mapping_back(bboxes, scale_factor, flip_horizontal, flip_vertical):
    """core/bbox/transforms.py:5-24 on a [N, >= 7] tensor or a box object with `.tensor` -> mapped copy (same type)"""
    t = getattr(bboxes, "tensor", bboxes)
    out = t.float().contiguous().clone()
    if out.shape[0]:
        mapping_back_(out, 1, out.shape[0], [scale_factor], [flip_horizontal], [flip_vertical])
    return type(bboxes)(out, box_dim=out.shape[-1]) if hasattr(bboxes, "tensor") else out


def merge_rows(boxes, scores, labels, test_cfg, num_classes, num_inputs=None):
    """the per-class NMS and top-max_num of merge_aug_bboxes_3d (merge_augs.py:58-101) on rows already mapped back:
    boxes [R, >= 7] float32, scores [R], labels [R] int32 (-1 = not a box); test_cfg keys use_rotate_nms, nms_thr,
    max_num (TTA_DEFAULTS where absent).  num_inputs: the number of boxes before NMS
    (len(aug_bboxes) of the reference) when known on the host; else read with the kept count in the one host read.
    -> boxes [K, D], scores [K], labels [K] (device), score descending; equal scores keep class order, then kept
    order (the reference's sort is not stable)."""
    R = boxes.shape[0]
    dev = boxes.device
    if R == 0:
        return boxes[:0], scores[:0], labels[:0]
    cfg = dict(TTA_DEFAULTS, **{k: test_cfg[k] for k in TTA_DEFAULTS if k in test_cfg})
    mode = "rotate" if cfg["use_rotate_nms"] else "normal"
    C = int(num_classes)
    _, idx, cnt = segmented_nms(boxes, scores, [mode] * C, [float(cfg["nms_thr"])] * C, R, labels=labels,
                                task_of_class=list(range(C)), box_format=BOX_LIDAR)
    valid = torch.arange(R, device=dev)[None, :] < cnt[:, None]                    # [C, R]
    rows = torch.where(valid, idx.long(), torch.zeros_like(idx, dtype=torch.long))
    key = torch.where(valid, scores.float()[rows], torch.full_like(rows, float("-inf"), dtype=torch.float32))
    order = torch.sort(key.view(-1), descending=True, stable=True).indices
    if num_inputs is None:
        kept, num_inputs = torch.stack([cnt.sum(), (labels >= 0).sum().to(cnt.dtype)]).tolist()   # the one host read
    else:
        kept = int(cnt.sum().item())
    num = min(int(cfg["max_num"]), int(num_inputs), int(kept))
    sel = rows.view(-1)[order[:num]]
    return boxes[sel], scores[sel], labels[sel]


def merge_aug_bboxes_3d(aug_results, img_metas, test_cfg, weighted_nms=False):
    """merge_augs.py:8-101: per view dict(boxes_3d, scores_3d, labels_3d) (boxes a [N, 7|9] tensor or a box object with
    `.tensor`) and its meta (a dict or a one-element list of one, with pcd_scale_factor / pcd_horizontal_flip /
    pcd_vertical_flip) -> dict(boxes_3d, scores_3d, labels_3d) on the device (the reference's bbox3d2result moves them to
    the CPU).  At most MAX_SEGMENT boxes over all views."""
    if weighted_nms:
        raise NotImplementedError("merge_aug_bboxes_3d: weighted_nms is not supported")
    assert len(aug_results) == len(img_metas), (len(aug_results), len(img_metas))
    metas = [m[0] if isinstance(m, (list, tuple)) else m for m in img_metas]
    boxes = [getattr(r["boxes_3d"], "tensor", r["boxes_3d"]).float() for r in aug_results]
    box_type = type(aug_results[0]["boxes_3d"]) if hasattr(aug_results[0]["boxes_3d"], "tensor") else None
    sizes = [b.shape[0] for b in boxes]
    cat = torch.cat(boxes, 0).contiguous()
    off = 0
    for b, m, n in zip(boxes, metas, sizes):     # one launch per view: the views' row counts differ
        if n:
            mapping_back_(cat[off:off + n], 1, n, [m["pcd_scale_factor"]], [m["pcd_horizontal_flip"]],
                          [m["pcd_vertical_flip"]])
        off += n
    scores = torch.cat([r["scores_3d"].float() for r in aug_results])
    labels = torch.cat([r["labels_3d"].to(torch.int32) for r in aug_results])
    if labels.numel() == 0:
        return dict(boxes_3d=aug_results[0]["boxes_3d"], scores_3d=scores, labels_3d=labels)
    num_classes = int(labels.max().item()) + 1       # range(max(labels) + 1), as the reference loops
    if num_classes > MAX_TASKS:
        raise _lib.IsfError(f"merge_aug_bboxes_3d: {num_classes} classes, at most {MAX_TASKS}")
    mb, ms, ml = merge_rows(cat, scores, labels, test_cfg, num_classes, num_inputs=sum(sizes))
    if box_type is not None:
        mb = box_type(mb, box_dim=mb.shape[-1])
    return dict(boxes_3d=mb, scores_3d=ms, labels_3d=ml)
