"""nuScenes detection evaluation (mAP / NDS) on the device: the step behind the reference config's
``evaluation = dict(interval=...)``.

The reference scores through ``NuScenesDataset._evaluate_single`` (mmdet3d/datasets/nuscenes_dataset.py:421-476): it
writes JSON and runs the nuScenes devkit on the host.  ``NuScenesDetectionEval`` consumes what
``TransFusionHeadV2.decode_and_nms`` leaves on the device and runs the same protocol in four kernel stages
(csrc/isf_eval.hip: match, order, curves, scalars).  ``update`` makes no host sync and no
device-to-host copy; ``compute`` makes one.

Everything is evaluated in the LiDAR frame (every metric is invariant under a rigid transform about z shared by
ground truth and predictions); ``lidar2ego`` serves the class-range filter only, as in the reference
(nuscenes_dataset.py:690-697).

Order rule (ours; the devkit's tie order is an accident of Python's sort): predictions are ordered by descending score,
ties by ascending (sample index, row index).  Parity with the devkit is by construction from its published protocol; it
is not measured here (tests/eval_common.py is the float64 restatement to hold against the devkit).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import IsfError

# nuscenes_dataset.py:70-112
DEFAULT_ATTRIBUTE = {
    "car": "vehicle.parked", "pedestrian": "pedestrian.moving", "trailer": "vehicle.parked", "truck": "vehicle.parked",
    "bus": "vehicle.moving", "motorcycle": "cycle.without_rider", "construction_vehicle": "vehicle.parked",
    "bicycle": "cycle.without_rider", "barrier": "", "traffic_cone": "",
}
ATTR_MAPPING = {
    "cycle.with_rider": 0, "cycle.without_rider": 1, "pedestrian.moving": 2, "pedestrian.standing": 3,
    "pedestrian.sitting_lying_down": 4, "vehicle.moving": 5, "vehicle.parked": 6, "vehicle.stopped": 7,
}
ERR_NAME_MAPPING = {"trans_err": "mATE", "scale_err": "mASE", "orient_err": "mAOE", "vel_err": "mAVE", "attr_err": "mAAE"}
CLASSES = ("car", "truck", "trailer", "bus", "construction_vehicle", "bicycle", "motorcycle", "pedestrian",
           "traffic_cone", "barrier")
TP_METRICS = ("trans_err", "scale_err", "orient_err", "vel_err", "attr_err")     # the devkit's order; the kernel's columns
# metrics that are NaN by definition (the devkit's calc_tp callers)
NAN_METRICS = {"traffic_cone": ("attr_err", "vel_err", "orient_err"), "barrier": ("attr_err", "vel_err")}
MAX_PRED, MAX_GT, MAX_CLASSES, MAX_THS, POINTS = 500, 1024, 31, 4, 101
_MOVING_VEHICLES = ("car", "construction_vehicle", "bus", "truck", "trailer")


def detection_cvpr_2019():
    """The devkit's detection_cvpr_2019 configuration as a dict of plain values."""
    return {
        "class_range": {"car": 50, "truck": 50, "bus": 50, "trailer": 50, "construction_vehicle": 50, "pedestrian": 40,
                        "motorcycle": 40, "bicycle": 40, "traffic_cone": 30, "barrier": 30},
        "dist_ths": [0.5, 1.0, 2.0, 4.0],
        "dist_th_tp": 2.0,
        "min_recall": 0.1,
        "min_precision": 0.1,
        "max_boxes_per_sample": 500,
        "mean_ap_weight": 5,
    }


def attribute_tables(class_names):
    """(moving, still): per class the attribute id of _format_bbox (nuscenes_dataset.py:378-397) for a speed above /
    not above 0.2 m/s; -1 where the attribute is ''."""
    moving, still = [], []
    for name in class_names:
        default = DEFAULT_ATTRIBUTE.get(name, "")
        if name in _MOVING_VEHICLES:
            mv = "vehicle.moving"
        elif name in ("bicycle", "motorcycle"):
            mv = "cycle.with_rider"
        else:
            mv = default
        if name == "pedestrian":
            sl = "pedestrian.standing"
        elif name == "bus":
            sl = "vehicle.stopped"
        else:
            sl = default
        moving.append(ATTR_MAPPING.get(mv, -1))
        still.append(ATTR_MAPPING.get(sl, -1))
    return moving, still


def _int_array(vals):
    return (ctypes.c_int * max(len(vals), 1))(*[int(v) for v in vals])


def predicted_attributes(labels, boxes, class_names):
    """The attribute heuristic of _format_bbox on the device (isf_eval_attributes): labels [...] int, boxes [..., 9] ->
    attribute ids [...] int32 (AttrMapping; -1 = no attribute).  No host sync."""
    _lib.require_cuda(labels, boxes)
    if boxes.shape[-1] < 9 or tuple(boxes.shape[:-1]) != tuple(labels.shape):
        raise IsfError(f"predicted_attributes: boxes {tuple(boxes.shape)} (velocity in columns 7-8) / labels "
                       f"{tuple(labels.shape)}")
    if not 1 <= len(class_names) <= MAX_CLASSES:
        raise IsfError(f"predicted_attributes: {len(class_names)} classes (1 .. {MAX_CLASSES})")
    b = boxes.float().contiguous()
    lab = labels.to(torch.int32).contiguous()
    out = torch.empty_like(lab)
    moving, still = attribute_tables(class_names)
    _lib.check(_lib.load().isf_eval_attributes(_lib.ptr(lab), _lib.ptr(b), b.shape[-1], lab.numel(), len(class_names),
                                               _int_array(moving), _int_array(still), _lib.ptr(out), _lib.stream()),
               "isf_eval_attributes")
    return out


class _Rows:
    """Device columns that grow geometrically; the number of used rows is host state.  Nothing is allocated before the
    first row arrives (a column without rows reads as None)."""

    def __init__(self, device, spec):
        self.device, self.spec, self.used, self.cap, self.cols = device, spec, 0, 0, {}

    def append(self, **new):
        n = int(next(iter(new.values())).shape[0])
        if n == 0:
            return
        if self.used + n > self.cap:
            cap = max(2 * self.cap, self.used + n, 1024)
            for k, (shape, dt) in self.spec.items():
                grown = torch.empty((cap,) + tuple(shape), dtype=dt, device=self.device)
                if self.used:
                    grown[:self.used] = self.cols[k][:self.used]
                self.cols[k] = grown
            self.cap = cap
        for k, v in new.items():
            self.cols[k][self.used:self.used + n] = v
        self.used += n

    def __getitem__(self, k):
        return self.cols.get(k)


class NuScenesDetectionEval:
    """nuScenes detection metrics over device tensors.

    ev.update(...) once per batch, ev.compute() -> the devkit's metrics_summary layout, ev.detail() -> the reference's
    flat keys (nuscenes_dataset.py:461-475), ev.reset().  Predictions are ordered by descending score, ties by ascending
    (sample index, row index) -- this project's rule, see the module docstring."""

    def __init__(self, class_names, config=None, device="cuda"):
        self.class_names = tuple(class_names)
        self.config = dict(config) if config is not None else detection_cvpr_2019()
        self.device = torch.device(device)
        cfg, C = self.config, len(self.class_names)
        if not 1 <= C <= MAX_CLASSES:
            raise IsfError(f"NuScenesDetectionEval: {C} classes (1 .. {MAX_CLASSES})")
        self.dist_ths = [float(t) for t in cfg["dist_ths"]]
        if not 1 <= len(self.dist_ths) <= MAX_THS or float(cfg["dist_th_tp"]) not in self.dist_ths:
            raise IsfError(f"NuScenesDetectionEval: dist_ths {self.dist_ths} (1 .. {MAX_THS} values, dist_th_tp among them)")
        if int(cfg["max_boxes_per_sample"]) > MAX_PRED:
            raise IsfError(f"NuScenesDetectionEval: max_boxes_per_sample {cfg['max_boxes_per_sample']} > {MAX_PRED}")
        missing = [n for n in self.class_names if n not in cfg["class_range"]]
        if missing:
            raise IsfError(f"NuScenesDetectionEval: no class_range for {missing}")
        self.tp_index = self.dist_ths.index(float(cfg["dist_th_tp"]))
        self._range = (ctypes.c_float * C)(*[float(cfg["class_range"][n]) for n in self.class_names])
        self._half_period = _int_array([n == "barrier" for n in self.class_names])
        self._nan_mask = _int_array([sum(1 << TP_METRICS.index(m) for m in NAN_METRICS.get(n, ())) for n in self.class_names])
        self._ths = (ctypes.c_double * len(self.dist_ths))(*self.dist_ths)
        self._points = None
        self.reset()

    def reset(self):
        dev = self.device
        self._pred = _Rows(dev, {"boxes": ((9,), torch.float32), "scores": ((), torch.float32), "labels": ((), torch.int32),
                                 "valid": ((), torch.uint8), "attrs": ((), torch.int32)})
        self._gt = _Rows(dev, {"boxes": ((9,), torch.float32), "labels": ((), torch.int32), "attrs": ((), torch.int32),
                               "num_pts": ((), torch.int32)})
        self._ego = _Rows(dev, {"m": ((16,), torch.float64)})
        self._pred_off, self._gt_off = [0], [0]
        self._metrics = None
        self.max_recall_ind = None
        self._tp_mask_rows = self._curves = None

    @property
    def num_samples(self):
        return len(self._pred_off) - 1

    def update(self, boxes, scores, labels, valid, gt_boxes, gt_labels, gt_attrs=None, gt_num_pts=None, pred_attrs=None,
               lidar2ego=None):
        """Append one batch.  boxes [B, P, 9] fp32, scores [B, P], labels [B, P] (decode_and_nms's outputs); valid: the
        [B, P] bool keep mask or the [B] int32 counts (rows [0, counts[b]) are the sample's result; None = every row);
        gt_boxes / gt_labels: one [G, 9] / [G] tensor per sample (head_loss.get_targets's layout); gt_attrs / pred_attrs:
        attribute ids, -1 = none (pred_attrs None: predicted_attributes); gt_num_pts: per sample [G] int, boxes with 0
        points are dropped; lidar2ego [B, 4, 4] (None: identity).  No host sync, no device-to-host copy: every size comes
        from the shapes."""
        gt_boxes = [g.tensor if hasattr(g, "tensor") else g for g in gt_boxes]
        if boxes.dim() != 3 or boxes.shape[-1] != 9:
            raise IsfError(f"update: boxes must be [B, P, 9], got {tuple(boxes.shape)}")
        B, P, _ = boxes.shape
        if P > MAX_PRED:
            raise IsfError(f"update: {P} predictions per sample; the evaluator takes at most {MAX_PRED} "
                           "(max_boxes_per_sample)")
        if tuple(scores.shape) != (B, P) or tuple(labels.shape) != (B, P):
            raise IsfError(f"update: scores {tuple(scores.shape)} / labels {tuple(labels.shape)} for boxes {tuple(boxes.shape)}")
        if len(gt_boxes) != B or len(gt_labels) != B:
            raise IsfError(f"update: {len(gt_boxes)} GT box sets / {len(gt_labels)} label sets for a batch of {B}")
        counts = [int(g.shape[0]) for g in gt_boxes]
        for g, lab in zip(gt_boxes, gt_labels):
            if g.dim() != 2 or g.shape[1] != 9 or int(lab.shape[0]) != int(g.shape[0]):
                raise IsfError(f"update: GT boxes must be [G, 9] with G labels, got {tuple(g.shape)} / {tuple(lab.shape)}")
        if max(counts, default=0) > MAX_GT:
            raise IsfError(f"update: {max(counts)} ground-truth boxes in one sample; the evaluator takes at most {MAX_GT}")
        _lib.require_cuda(boxes, scores, labels, valid, pred_attrs, lidar2ego, *gt_boxes, *gt_labels,
                          *(gt_attrs or ()), *(gt_num_pts or ()))
        dev = self.device
        if valid is None:
            mask = torch.ones((B, P), dtype=torch.uint8, device=dev)
        elif valid.dim() == 2:
            if tuple(valid.shape) != (B, P):
                raise IsfError(f"update: keep mask {tuple(valid.shape)} for boxes {tuple(boxes.shape)}")
            mask = (valid != 0).to(torch.uint8)
        else:
            if tuple(valid.shape) != (B,):
                raise IsfError(f"update: counts {tuple(valid.shape)} for a batch of {B}")
            mask = (torch.arange(P, device=dev)[None, :] < valid.to(dev)[:, None]).to(torch.uint8)
        if pred_attrs is None:
            pred_attrs = predicted_attributes(labels, boxes, self.class_names)
        elif tuple(pred_attrs.shape) != (B, P):
            raise IsfError(f"update: pred_attrs {tuple(pred_attrs.shape)} for boxes {tuple(boxes.shape)}")
        self._pred.append(boxes=boxes.reshape(B * P, 9), scores=scores.reshape(-1), labels=labels.reshape(-1),
                          valid=mask.reshape(-1), attrs=pred_attrs.reshape(-1))
        G = sum(counts)
        if G:
            cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])    # noqa: E731
            for name, vals in (("gt_attrs", gt_attrs), ("gt_num_pts", gt_num_pts)):
                if vals is not None and [int(v.shape[0]) for v in vals] != counts:
                    raise IsfError(f"update: {name} does not match the GT boxes")
            attrs = cat(gt_attrs) if gt_attrs is not None else torch.full((G,), -1, dtype=torch.int32, device=dev)
            npts = cat(gt_num_pts) if gt_num_pts is not None else torch.ones(G, dtype=torch.int32, device=dev)
            self._gt.append(boxes=torch.cat(list(gt_boxes)), labels=cat(gt_labels), attrs=attrs, num_pts=npts)
        if lidar2ego is None:
            ego = torch.eye(4, dtype=torch.float64, device=dev).reshape(1, 16).expand(B, 16)
        else:
            if tuple(lidar2ego.shape) != (B, 4, 4):
                raise IsfError(f"update: lidar2ego {tuple(lidar2ego.shape)} for a batch of {B}")
            ego = lidar2ego.reshape(B, 16)
        self._ego.append(m=ego)
        for b in range(B):
            self._pred_off.append(self._pred_off[-1] + P)
            self._gt_off.append(self._gt_off[-1] + counts[b])
        self._metrics = None

    # ------------------------------------------------------------------------------------------------ the four stages
    def _run(self):
        """The four stages on the current stream -> (result fp64 device block, curves, tp_mask_rows); no host sync."""
        lib, dev, st = _lib.load(), self.device, _lib.stream()
        C, T, S, R = len(self.class_names), len(self.dist_ths), self.num_samples, self._pred.used
        if self._points is None:
            self._points = torch.from_numpy(np.linspace(0, 1, POINTS)).to(dev)     # host values, uploaded as fp64
        poff = torch.tensor(self._pred_off, dtype=torch.int32).to(dev)
        goff = torch.tensor(self._gt_off, dtype=torch.int32).to(dev)
        max_pred = max((b - a for a, b in zip(self._pred_off, self._pred_off[1:])), default=0)
        max_gt = max((b - a for a, b in zip(self._gt_off, self._gt_off[1:])), default=0)
        n = max(R, 1)
        keys = torch.empty(n, dtype=torch.int32, device=dev)
        cls = torch.empty(n, dtype=torch.int32, device=dev)
        tp_mask = torch.empty(n, dtype=torch.uint8, device=dev)
        tp_rows = torch.empty(n, dtype=torch.uint8, device=dev)
        conf = torch.empty(n, dtype=torch.float64, device=dev)
        errs = torch.empty((n, len(TP_METRICS)), dtype=torch.float64, device=dev)
        counts = torch.empty(2 * C, dtype=torch.int32, device=dev)
        order = torch.empty(n, dtype=torch.int32, device=dev)
        curves = torch.empty((C, 2 * T + len(TP_METRICS), POINTS), dtype=torch.float64, device=dev)
        result = torch.empty(C * T + C * len(TP_METRICS) + 2 * C + 2 * len(TP_METRICS) + 2, dtype=torch.float64, device=dev)
        p, g = self._pred, self._gt
        _lib.check(lib.isf_eval_match(
            _lib.ptr(p["boxes"]), _lib.ptr(p["scores"]), _lib.ptr(p["labels"]), _lib.ptr(p["valid"]), _lib.ptr(p["attrs"]),
            _lib.ptr(poff), max_pred, _lib.ptr(g["boxes"]), _lib.ptr(g["labels"]), _lib.ptr(g["attrs"]),
            _lib.ptr(g["num_pts"]), _lib.ptr(goff), max_gt, _lib.ptr(self._ego["m"]), S, C, self._range, self._half_period,
            self._ths, T, self.tp_index, _lib.ptr(keys), _lib.ptr(cls), _lib.ptr(tp_mask), _lib.ptr(tp_rows),
            _lib.ptr(conf), _lib.ptr(errs), _lib.ptr(counts), st), "isf_eval_match")
        _lib.check(lib.isf_eval_order(_lib.ptr(keys), _lib.ptr(cls), R, C, _lib.ptr(order), st), "isf_eval_order")
        _lib.check(lib.isf_eval_curves(_lib.ptr(order), _lib.ptr(tp_mask), _lib.ptr(conf), _lib.ptr(errs), _lib.ptr(counts),
                                       _lib.ptr(self._points), R, C, T, self.tp_index, _lib.ptr(curves), st),
                   "isf_eval_curves")
        cfg = self.config
        _lib.check(lib.isf_eval_scalars(_lib.ptr(curves), C, T, self.tp_index, self._nan_mask, float(cfg["min_recall"]),
                                        float(cfg["min_precision"]), float(cfg["mean_ap_weight"]), _lib.ptr(result), st),
                   "isf_eval_scalars")
        return result, curves, tp_rows[:R]

    def compute(self):
        """-> the devkit's metrics_summary layout: label_aps[class][dist_th], label_tp_errors[class][metric],
        mean_dist_aps[class], mean_ap, tp_errors[metric], tp_scores[metric], nd_score.  One copy of one small fp64 block
        (the only sync).  Afterwards max_recall_ind[class] holds the last recall point with a non-zero confidence at
        dist_th_tp."""
        result, self._curves, self._tp_mask_rows = self._run()
        r = result.cpu().numpy()
        C, T, E = len(self.class_names), len(self.dist_ths), len(TP_METRICS)
        ap = r[:C * T].reshape(C, T)
        tp = r[C * T:C * T + C * E].reshape(C, E)
        o = C * T + C * E
        mda, mri, tpe, tps = r[o:o + C], r[o + C:o + 2 * C], r[o + 2 * C:o + 2 * C + E], r[o + 2 * C + E:o + 2 * C + 2 * E]
        names = self.class_names
        self.max_recall_ind = {n: int(mri[i]) for i, n in enumerate(names)}
        self._metrics = {
            "label_aps": {n: {t: float(ap[i, j]) for j, t in enumerate(self.dist_ths)} for i, n in enumerate(names)},
            "label_tp_errors": {n: {m: float(tp[i, j]) for j, m in enumerate(TP_METRICS)} for i, n in enumerate(names)},
            "mean_dist_aps": {n: float(mda[i]) for i, n in enumerate(names)},
            "mean_ap": float(r[o + 2 * C + 2 * E]),
            "tp_errors": {m: float(tpe[j]) for j, m in enumerate(TP_METRICS)},
            "tp_scores": {m: float(tps[j]) for j, m in enumerate(TP_METRICS)},
            "nd_score": float(r[o + 2 * C + 2 * E + 1]),
        }
        return self._metrics

    def tp_masks(self):
        """After compute(): uint8 [rows] on the device, one per prediction row in update order (sample by sample, P rows
        each); bit t = true positive at dist_ths[t], 0 for dropped rows."""
        if self._tp_mask_rows is None:
            raise IsfError("tp_masks: call compute() first")
        return self._tp_mask_rows

    def curves(self):
        """After compute(): fp64 [classes, 2 * T + 5, 101] on the device: precision per threshold, confidence per
        threshold, the five TP error curves at dist_th_tp."""
        if self._tp_mask_rows is None:
            raise IsfError("curves: call compute() first")
        return self._curves

    def detail(self, result_name="pts_bbox"):
        """The reference's flat dict (nuscenes_dataset.py:461-475): AP and error values rounded through
        float('{:.4f}'.format(v)), NDS and mAP as they are."""
        m = self._metrics if self._metrics is not None else self.compute()
        prefix = f"{result_name}_NuScenes"
        detail = {}
        for name in self.class_names:
            for k, v in m["label_aps"][name].items():
                detail[f"{prefix}/{name}_AP_dist_{k}"] = float("{:.4f}".format(v))
            for k, v in m["label_tp_errors"][name].items():
                detail[f"{prefix}/{name}_{k}"] = float("{:.4f}".format(v))
            for k, v in m["tp_errors"].items():
                detail[f"{prefix}/{ERR_NAME_MAPPING[k]}"] = float("{:.4f}".format(v))
        detail[f"{prefix}/NDS"] = m["nd_score"]
        detail[f"{prefix}/mAP"] = m["mean_ap"]
        return detail
