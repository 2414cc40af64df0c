"""Float64 numpy restatement of the nuScenes detection protocol as isfusion_amd.evaluation builds it (DESIGN.md section
4.0f), seeded problem generators, the guard of the GPU comparisons and the helpers that feed a problem to the evaluator.

A problem is a list of samples; a sample is a dict of numpy arrays: boxes [P, 9] f32, scores [P] f32, labels [P] i32,
valid [P] bool, attrs [P] i32 (-1 = none), gt_boxes [G, 9] f32, gt_labels [G] i32, gt_attrs [G] i32, gt_num_pts [G] i32,
lidar2ego [4, 4] f64.  Box layout: x, y, z_bottom, dx, dy, dz, yaw, vx, vy.

This file is the thing to hold against the nuScenes devkit on a machine that has it: np.interp, np.cumsum and
np.nancumsum are used literally where the devkit uses them."""
import numpy as np

CLASSES = ("car", "truck", "trailer", "bus", "construction_vehicle", "bicycle", "motorcycle", "pedestrian",
           "traffic_cone", "barrier")
TP_METRICS = ("trans_err", "scale_err", "orient_err", "vel_err", "attr_err")
CONFIG = {
    "class_range": {"car": 50, "truck": 50, "bus": 50, "trailer": 50, "construction_vehicle": 50, "pedestrian": 40,
                    "motorcycle": 40, "bicycle": 40, "traffic_cone": 30, "barrier": 30},
    "dist_ths": [0.5, 1.0, 2.0, 4.0], "dist_th_tp": 2.0, "min_recall": 0.1, "min_precision": 0.1,
    "max_boxes_per_sample": 500, "mean_ap_weight": 5,
}
# nuscenes_dataset.py:70-91
DEFAULT_ATTRIBUTE = {"car": "vehicle.parked", "pedestrian": "pedestrian.moving", "trailer": "vehicle.parked",
                     "truck": "vehicle.parked", "bus": "vehicle.moving", "motorcycle": "cycle.without_rider",
                     "construction_vehicle": "vehicle.parked", "bicycle": "cycle.without_rider", "barrier": "",
                     "traffic_cone": ""}
ATTR_MAPPING = {"cycle.with_rider": 0, "cycle.without_rider": 1, "pedestrian.moving": 2, "pedestrian.standing": 3,
                "pedestrian.sitting_lying_down": 4, "vehicle.moving": 5, "vehicle.parked": 6, "vehicle.stopped": 7}
NUM_POINTS = 101


# ------------------------------------------------------------------------------------------------------ restatement
def predicted_attribute(name, vx, vy):
    """_format_bbox, nuscenes_dataset.py:378-397, for one box -> attribute id (-1 for '')"""
    if np.sqrt(float(vx) ** 2 + float(vy) ** 2) > 0.2:
        if name in ["car", "construction_vehicle", "bus", "truck", "trailer"]:
            attr = "vehicle.moving"
        elif name in ["bicycle", "motorcycle"]:
            attr = "cycle.with_rider"
        else:
            attr = DEFAULT_ATTRIBUTE[name]
    else:
        if name in ["pedestrian"]:
            attr = "pedestrian.standing"
        elif name in ["bus"]:
            attr = "vehicle.stopped"
        else:
            attr = DEFAULT_ATTRIBUTE[name]
    return ATTR_MAPPING.get(attr, -1)


def ego_radius(box, lidar2ego):
    b = np.asarray(box, np.float64)
    m = np.asarray(lidar2ego, np.float64)
    c = np.array([b[0], b[1], b[2] + b[5] * 0.5])
    ex = m[0, 0] * c[0] + m[0, 1] * c[1] + m[0, 2] * c[2] + m[0, 3]
    ey = m[1, 0] * c[0] + m[1, 1] * c[1] + m[1, 2] * c[2] + m[1, 3]
    return float(np.sqrt(ex * ex + ey * ey))


def _kept(boxes, labels, extra, lidar2ego, ranges):
    keep = np.zeros(len(labels), bool)
    for i, lab in enumerate(labels):
        if not extra[i] or lab < 0 or lab >= len(ranges):
            continue
        keep[i] = not (ego_radius(boxes[i], lidar2ego) > ranges[lab])
    return keep


def angle_diff(x, y, period):
    diff = (x - y + period / 2) % period - period / 2
    if diff > np.pi:
        diff = diff - (2 * np.pi)
    return diff


def match_errors(gt, pred, gt_attr, pred_attr, name):
    gt, pred = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    inter = np.prod(np.minimum(gt[3:6], pred[3:6]))
    union = np.prod(gt[3:6]) + np.prod(pred[3:6]) - inter
    period = np.pi if name == "barrier" else 2 * np.pi
    return {
        "trans_err": float(np.linalg.norm(gt[:2] - pred[:2])),
        "vel_err": float(np.linalg.norm(gt[7:9] - pred[7:9])),
        "scale_err": float(1 - inter / union),
        "orient_err": float(abs(angle_diff(gt[6], pred[6], period))),
        "attr_err": float("nan") if gt_attr < 0 else float(1 - (gt_attr == pred_attr)),
    }


def cummean(x):
    x = np.asarray(x, np.float64)
    if sum(np.isnan(x)) == len(x):
        return np.ones(len(x))
    sum_vals = np.nancumsum(x.astype(float))
    count_vals = np.cumsum(~np.isnan(x))
    return np.divide(sum_vals, count_vals, out=np.zeros_like(sum_vals), where=count_vals != 0)


def no_predictions():
    return {"precision": np.zeros(NUM_POINTS), "confidence": np.zeros(NUM_POINTS),
            **{m: np.ones(NUM_POINTS) for m in TP_METRICS}}


def evaluate(samples, class_names=CLASSES, config=CONFIG):
    """-> dict(metrics = the devkit's metrics_summary layout, tp_masks = one uint8 [P] per sample (bit t: TP at
    dist_ths[t]), max_recall_ind = {class: int}, curves = {class: {dist_th: metric data}})"""
    ranges = [float(config["class_range"][n]) for n in class_names]
    ths = [float(t) for t in config["dist_ths"]]
    points = np.linspace(0, 1, NUM_POINTS)
    pk = [_kept(s["boxes"], s["labels"], s["valid"] & ~np.isnan(s["scores"]), s["lidar2ego"], ranges) for s in samples]
    gk = [_kept(s["gt_boxes"], s["gt_labels"], s["gt_num_pts"] > 0, s["lidar2ego"], ranges) for s in samples]
    tp_masks = [np.zeros(len(s["labels"]), np.uint8) for s in samples]
    curves, max_recall_ind = {}, {}
    for c, name in enumerate(class_names):
        npos = sum(int((gk[si] & (s["gt_labels"] == c)).sum()) for si, s in enumerate(samples))
        preds = [(float(s["scores"][i]), si, i) for si, s in enumerate(samples) for i in range(len(s["labels"]))
                 if pk[si][i] and s["labels"][i] == c]
        preds.sort(key=lambda p: (-p[0], p[1], p[2]))          # descending score, ties by (sample, row)
        gts = {si: np.nonzero(gk[si] & (s["gt_labels"] == c))[0] for si, s in enumerate(samples)}
        gxy = {si: s["gt_boxes"][gts[si], :2].astype(np.float64) for si, s in enumerate(samples)}
        curves[name] = {}
        for t, th in enumerate(ths):
            taken = {si: np.zeros(len(g), bool) for si, g in gts.items()}
            tp, fp, conf = [], [], []
            match = {m: [] for m in TP_METRICS}
            match["conf"] = []
            for score, si, i in preds:
                s = samples[si]
                best, bg = np.inf, None
                if len(gts[si]):
                    d = np.linalg.norm(gxy[si] - s["boxes"][i, :2].astype(np.float64), axis=1)
                    d = np.where(taken[si], np.inf, d)
                    bg = int(np.argmin(d))                     # the first box wins a tie
                    best = d[bg]
                if best < th:
                    taken[si][bg] = True
                    tp.append(1)
                    fp.append(0)
                    tp_masks[si][i] |= 1 << t
                    if th == config["dist_th_tp"]:
                        g = gts[si][bg]
                        e = match_errors(s["gt_boxes"][g], s["boxes"][i], int(s["gt_attrs"][g]), int(s["attrs"][i]), name)
                        for m in TP_METRICS:
                            match[m].append(e[m])
                        match["conf"].append(score)
                else:
                    tp.append(0)
                    fp.append(1)
                conf.append(score)
            if npos == 0 or sum(tp) == 0:
                curves[name][th] = no_predictions()
                continue
            tpc, fpc, conf = np.cumsum(tp).astype(float), np.cumsum(fp).astype(float), np.array(conf)
            prec, rec = tpc / (fpc + tpc), tpc / float(npos)
            md = {"precision": np.interp(points, rec, prec, right=0), "confidence": np.interp(points, rec, conf, right=0)}
            for m in TP_METRICS:
                if th == config["dist_th_tp"]:
                    md[m] = np.interp(md["confidence"][::-1], np.array(match["conf"])[::-1], cummean(match[m])[::-1])[::-1]
                else:
                    md[m] = np.ones(NUM_POINTS)                # never read
            curves[name][th] = md
    first = round(100 * config["min_recall"]) + 1
    label_aps, label_tp = {}, {}
    for name in class_names:
        label_aps[name] = {}
        for th in ths:
            prec = np.copy(curves[name][th]["precision"])[first:]
            prec -= config["min_precision"]
            prec[prec < 0] = 0
            label_aps[name][th] = float(np.mean(prec)) / (1.0 - config["min_precision"])
        md = curves[name][float(config["dist_th_tp"])]
        nz = np.nonzero(md["confidence"])[0]
        last = 0 if len(nz) == 0 else int(nz[-1])
        max_recall_ind[name] = last
        label_tp[name] = {}
        for m in TP_METRICS:
            if name == "traffic_cone" and m in ("attr_err", "vel_err", "orient_err"):
                v = float("nan")
            elif name == "barrier" and m in ("attr_err", "vel_err"):
                v = float("nan")
            elif last < first:
                v = 1.0
            else:
                v = float(np.mean(md[m][first:last + 1]))
            label_tp[name][m] = v
    mean_dist_aps = {n: float(np.mean(list(v.values()))) for n, v in label_aps.items()}
    mean_ap = float(np.mean(list(mean_dist_aps.values())))
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            tp_errors = {m: float(np.nanmean([label_tp[n][m] for n in class_names])) for m in TP_METRICS}
    tp_scores = {m: max(1.0 - tp_errors[m], 0.0) for m in TP_METRICS}
    total = float(config["mean_ap_weight"] * mean_ap + np.sum(list(tp_scores.values())))
    nd_score = total / float(config["mean_ap_weight"] + len(tp_scores))
    metrics = {"label_aps": label_aps, "label_tp_errors": label_tp, "mean_dist_aps": mean_dist_aps, "mean_ap": mean_ap,
               "tp_errors": tp_errors, "tp_scores": tp_scores, "nd_score": nd_score}
    return {"metrics": metrics, "tp_masks": tp_masks, "max_recall_ind": max_recall_ind, "curves": curves}


# ------------------------------------------------------------------------------------------------------- generators
def _box(xy, size, yaw, vel, z=-1.0):
    return np.array([xy[0], xy[1], z, size[0], size[1], size[2], yaw, vel[0], vel[1]], np.float32)


def make_sample(boxes, scores, labels, gt_boxes, gt_labels, valid=None, attrs=None, gt_attrs=None, gt_num_pts=None,
                lidar2ego=None, class_names=CLASSES):
    boxes = np.asarray(boxes, np.float32).reshape(-1, 9)
    labels = np.asarray(labels, np.int32).reshape(-1)
    gt_boxes = np.asarray(gt_boxes, np.float32).reshape(-1, 9)
    gt_labels = np.asarray(gt_labels, np.int32).reshape(-1)
    if attrs is None:
        attrs = [predicted_attribute(class_names[c], b[7], b[8]) if 0 <= c < len(class_names) else -1
                 for c, b in zip(labels, boxes)]
    return {
        "boxes": boxes, "scores": np.asarray(scores, np.float32).reshape(-1), "labels": labels,
        "valid": np.ones(len(labels), bool) if valid is None else np.asarray(valid, bool),
        "attrs": np.asarray(attrs, np.int32).reshape(-1), "gt_boxes": gt_boxes, "gt_labels": gt_labels,
        "gt_attrs": np.full(len(gt_labels), -1, np.int32) if gt_attrs is None else np.asarray(gt_attrs, np.int32),
        "gt_num_pts": np.ones(len(gt_labels), np.int32) if gt_num_pts is None else np.asarray(gt_num_pts, np.int32),
        "lidar2ego": np.eye(4) if lidar2ego is None else np.asarray(lidar2ego, np.float64),
    }


def rigid(yaw, t):
    m = np.eye(4)
    m[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    m[:3, 3] = t
    return m


def distinct_scores(rng, n):
    """n distinct fp32 scores in (0, 1), shuffled"""
    s = ((rng.permutation(n) + 1.0) / (n + 1.0)).astype(np.float32)
    assert len(np.unique(s)) == n
    return s


def random_problem(seed, S, P, max_gt, classes=tuple(range(10)), extent=48.0, prefix_valid=False, ego=True):
    """predictions = ground truth + noise (several noise scales, so that every threshold decides something) + clutter;
    distinct scores; some GT boxes without points or without attribute; a z-rotation + translation as lidar2ego"""
    rng = np.random.default_rng(seed)
    scores = distinct_scores(rng, S * P).reshape(S, P)
    out = []
    for si in range(S):
        G = int(rng.integers(max(1, max_gt // 2), max_gt + 1))
        gl = rng.choice(classes, G).astype(np.int32)
        gb = np.stack([_box(rng.uniform(-extent, extent, 2), rng.uniform(0.4, 5.0, 3), rng.uniform(-np.pi, np.pi),
                            rng.normal(0, 1.5, 2) * (rng.random() < 0.6)) for _ in range(G)])
        ga = rng.integers(-1, 8, G).astype(np.int32)
        gn = rng.integers(0, 12, G).astype(np.int32)
        pb, pl, quality = [], [], []
        for g in range(G):
            if len(pb) < P and rng.random() < 0.85:
                quality.append(0.7 + rng.random())
                b = gb[g].copy()
                b[:2] += rng.normal(0, rng.choice([0.1, 0.4, 1.0, 2.5]), 2).astype(np.float32)
                b[3:6] *= rng.uniform(0.8, 1.25, 3).astype(np.float32)
                b[6] += np.float32(rng.normal(0, 0.3))
                b[7:9] += rng.normal(0, 0.3, 2).astype(np.float32)
                pb.append(b)
                pl.append(gl[g] if rng.random() < 0.9 else rng.choice(classes))
        while len(pb) < P:
            pb.append(_box(rng.uniform(-extent, extent, 2), rng.uniform(0.4, 5.0, 3), rng.uniform(-np.pi, np.pi),
                           rng.normal(0, 1.0, 2)))
            pl.append(rng.choice(classes))
            quality.append(rng.random())
        sc = np.empty(P, np.float32)
        sc[np.argsort(-np.asarray(quality))] = np.sort(scores[si])[::-1]     # predictions near a box tend to score higher
        perm = rng.permutation(P)
        pb, pl, sc = np.stack(pb)[perm], np.asarray(pl, np.int32)[perm], sc[perm]
        if prefix_valid:
            valid = np.arange(P) < int(rng.integers(P // 2, P + 1))
        else:
            valid = rng.random(P) < 0.9
        m = rigid(rng.uniform(-np.pi, np.pi), [rng.uniform(-2, 2), rng.uniform(-2, 2), 1.8]) if ego else None
        out.append(make_sample(pb, sc, pl, gb, gl, valid=valid, gt_attrs=ga, gt_num_pts=gn, lidar2ego=m))
    return out


def small_problem(seed=11):
    """S = 3, P = 40, <= 12 boxes per sample, all ten classes, with the special cases of the small GPU test"""
    rng = np.random.default_rng(seed)
    S, P = 3, 40
    scores = distinct_scores(rng, S * P).reshape(S, P)
    ego = [rigid(0.7, [1.5, -0.8, 1.8]), rigid(-2.1, [0.3, 2.2, 1.7]), rigid(3.0, [-1.1, 0.4, 1.9])]
    out = []
    for si in range(S):
        gb, gl, ga, gn, pb, pl = [], [], [], [], [], []

        def add(label, xy, yaw=0.3, vel=(0.0, 0.0), attr=-1, npts=5, pred_shift=None, pred_yaw=None, size=(1.5, 1.0, 1.2)):
            b = _box(xy, size, yaw, vel)
            gb.append(b), gl.append(label), ga.append(attr), gn.append(npts)
            if pred_shift is not None:
                p = b.copy()
                p[:2] += np.asarray(pred_shift, np.float32)
                p[3:6] *= np.float32(1.1)
                p[6] = np.float32(yaw if pred_yaw is None else pred_yaw)
                p[7:9] += np.float32(0.25)
                pb.append(p), pl.append(label)
        add(0, (5 + si, 3), vel=(1.0, 0.5), attr=5, pred_shift=(0.2, 0.1))                # car, matched at every threshold
        add(0, (-12, 7 + si), attr=-1, pred_shift=(0.7, 0.0))                           # NaN-attribute ground truth
        add(1, (15, -9 + si), attr=6, pred_shift=(1.2, 0.9))                             # truck, matched at 2.0 / 4.0
        add(2, (-20, -15), attr=6)                                                      # trailer: ground truth, no predictions
        add(3, (8, 22), vel=(0.0, 0.0), attr=7, pred_shift=(0.1, -0.3))                  # bus, still -> vehicle.stopped
        add(5, (-6, -4), vel=(1.0, 1.0), attr=0, pred_shift=(0.3, 0.3))                  # bicycle
        add(6, (11 + si, 11), attr=1, pred_shift=(2.1, 2.2))                             # motorcycle: > 0.5 .. 2.0, < 4.0
        add(7, (2, -9), vel=(0.5, 0.0), attr=2, pred_shift=(0.05, 0.02))                 # pedestrian
        add(7, (3, -10), attr=3, npts=0, pred_shift=(0.02, 0.05))                        # a ground-truth box with 0 points
        add(8, (-4, 12), pred_shift=(0.2, 0.2))                                         # traffic_cone
        add(9, (7, -14 - si), yaw=0.1, pred_shift=(0.1, 0.1), pred_yaw=0.1 + np.pi - 0.02)    # barrier: yaw apart by ~pi
        add(9, (9, -17), yaw=-1.0, pred_shift=(0.3, 0.1), pred_yaw=-1.0 - np.pi / 2)
        # both sides of the class range through the sample's lidar2ego: the centre at ego radius range -+ 0.5 m
        inv = np.linalg.inv(ego[si])
        for label, r in ((8, 29.5), (8, 30.5), (7, 39.5), (7, 40.5)):
            ang = 0.4 * label + r
            c = inv @ np.array([r * np.cos(ang), r * np.sin(ang), 1.8 - 1.0 + 0.6, 1.0])
            if len(gb) < 12:
                add(label, c[:2], pred_shift=(0.1, 0.0))
            else:
                pb.append(_box(c[:2], (1.5, 1.0, 1.2), 0.3, (0, 0))), pl.append(label)
        while len(pb) < P:                                                              # clutter: construction_vehicle has no
            pb.append(_box(rng.uniform(-45, 45, 2), rng.uniform(0.5, 4, 3), rng.uniform(-3, 3), rng.normal(0, 1, 2)))
            pl.append(int(rng.choice([0, 1, 3, 4, 4, 5, 6, 7, 8, 9])))                  # ground truth anywhere
        perm = rng.permutation(P)
        pb, pl = np.stack(pb)[perm], np.asarray(pl, np.int32)[perm]
        valid = np.ones(P, bool)
        valid[rng.choice(P, 3, replace=False)] = False
        assert len(gb) <= 12
        out.append(make_sample(pb, scores[si], pl, np.stack(gb), gl, valid=valid, gt_attrs=ga, gt_num_pts=gn,
                               lidar2ego=ego[si]))
    return out


def deep_problem(seed=31):
    """one sample, 500 predictions of one class, 70 ground-truth boxes of that class"""
    rng = np.random.default_rng(seed)
    G, P = 70, 500
    gb = np.stack([_box(rng.uniform(-30, 30, 2), rng.uniform(1, 5, 3), rng.uniform(-3, 3), rng.normal(0, 1, 2)) for _ in range(G)])
    pb = []
    for i in range(P):
        b = gb[i % G].copy()
        b[:2] += rng.normal(0, [0.2, 0.8, 1.5, 3.0, 6.0, 9.0, 12.0, 15.0][i // G], 2).astype(np.float32)
        b[3:6] *= rng.uniform(0.8, 1.25, 3).astype(np.float32)
        b[6] += np.float32(rng.normal(0, 0.5))
        pb.append(b)
    sc = np.empty(P, np.float32)
    sc[np.argsort(np.arange(P) // G + 2.0 * rng.random(P))] = np.sort(distinct_scores(rng, P))[::-1]   # closer = higher, loosely
    perm = rng.permutation(P)
    return [make_sample(np.stack(pb)[perm], sc[perm], np.zeros(P, np.int32), gb, np.zeros(G, np.int32),
                        gt_attrs=rng.integers(-1, 8, G))]


def tie_problem(seed=41):
    """duplicated scores within and across samples: six score values over 4 x 30 predictions of two classes"""
    rng = np.random.default_rng(seed)
    out = random_problem(seed, 4, 30, 10, classes=(0, 7), extent=20.0, ego=False)
    levels = np.array([0.9, 0.75, 0.6, 0.45, 0.3, 0.15], np.float32)
    for s in out:
        s["scores"] = levels[np.minimum(((1.0 - s["scores"]) * len(levels)).astype(int), len(levels) - 1)]
    return out


def negative_problem(seed=61):
    """scores on both sides of zero (the head produces none below; the evaluator orders them all the same)"""
    out = random_problem(seed, 3, 30, 8, classes=(0, 1, 7), extent=25.0)
    for s in out:
        s["scores"] = (s["scores"] - np.float32(0.5)).astype(np.float32)
    return out


def perfect_problem():
    """(a): predictions equal to the ground truth, attributes included, over all ten classes"""
    rng = np.random.default_rng(5)
    out, scores = [], distinct_scores(rng, 40).reshape(2, 20)
    for si in range(2):
        gl = np.arange(10, dtype=np.int32).repeat(2)
        gb = np.stack([_box(rng.uniform(-20, 20, 2), rng.uniform(0.5, 4, 3), rng.uniform(-3, 3), rng.normal(0, 1, 2)) for _ in gl])
        ga = rng.integers(0, 8, len(gl)).astype(np.int32)
        out.append(make_sample(gb.copy(), scores[si], gl, gb, gl, attrs=ga, gt_attrs=ga))
    return out


def empty_problem():
    """(b): no valid prediction"""
    out = perfect_problem()
    for s in out:
        s["valid"][:] = False
    return out


def hand_problem():
    """(c): one class, npos = 2; (score, distance to the nearest box) = (0.9, 0.3), (0.8, none within 4 m), (0.7, 0.6 to
    the other box)"""
    size, z = (4.0, 2.0, 1.5), (0.0, 0.0)
    gb = [_box((0, 0), size, 0.0, z), _box((10, 0), size, 0.0, z)]
    pb = [_box((0.3, 0), size, 0.0, z), _box((30, 30), size, 0.0, z), _box((10.6, 0), size, 0.0, z)]
    return [make_sample(pb, [0.9, 0.8, 0.7], [0, 0, 0], gb, [0, 0])]


# ------------------------------------------------------------------------------------------------------------ guard
def guard(samples, class_names=CLASSES, config=CONFIG, allow_ties=False, margin=1e-6):
    """the conditions the GPU comparisons rest on: no ground-truth--prediction distance within `margin` of a threshold,
    no ego radius within `margin` of a class range, no duplicate scores (unless allow_ties)"""
    ths = np.asarray(config["dist_ths"], np.float64)
    scores = []
    for s in samples:
        pred = s["boxes"][s["valid"]]                         # rows that are not valid may hold anything
        if len(s["gt_boxes"]) and len(pred):
            d = np.linalg.norm(s["gt_boxes"][:, None, :2].astype(np.float64) - pred[None, :, :2].astype(np.float64), axis=2)
            gap = np.abs(d[..., None] - ths).min()
            assert gap > margin, f"a distance lies {gap:.2e} from a threshold"
        for boxes, labels in ((pred, s["labels"][s["valid"]]), (s["gt_boxes"], s["gt_labels"])):
            for b, c in zip(boxes, labels):
                if 0 <= c < len(class_names):
                    gap = abs(ego_radius(b, s["lidar2ego"]) - config["class_range"][class_names[c]])
                    assert gap > margin, f"an ego radius lies {gap:.2e} from its class range"
        scores.append(s["scores"][s["valid"]])
    scores = np.concatenate(scores) if scores else np.zeros(0)
    if not allow_ties:
        assert len(np.unique(scores)) == len(scores), "duplicate scores"
    return True


# the seeds / problems of tests/test_gpu_eval.py; tests/test_eval.py holds the guard over every one of them
WIDE_SEED, E2E_SEED = 21, 51
GPU_PROBLEMS = {
    "small": lambda: small_problem(11),
    "wide": lambda: random_problem(WIDE_SEED, 64, 200, 12),
    "deep": lambda: deep_problem(31),
    "ties": lambda: tie_problem(41),
    "negative": lambda: negative_problem(61),
    "perfect": perfect_problem,
    "empty": empty_problem,
    "hand": hand_problem,
}


# ------------------------------------------------------------------------------------------------- evaluator helpers
def feed(ev, samples, batch=None, counts=False, device="cuda"):
    """update() the evaluator with the problem, `batch` samples per call (all samples have the same P).  counts: pass
    `valid` as per-sample counts (the valid masks must be prefixes)."""
    import torch
    batch = batch or len(samples)
    for b0 in range(0, len(samples), batch):
        ss = samples[b0:b0 + batch]
        t = lambda k, dt: torch.from_numpy(np.stack([s[k] for s in ss])).to(device=device, dtype=dt)   # noqa: E731
        if counts:
            for s in ss:
                n = int(s["valid"].sum())
                assert s["valid"][:n].all()
            valid = torch.tensor([int(s["valid"].sum()) for s in ss], dtype=torch.int32, device=device)
        else:
            valid = t("valid", torch.bool)
        g = lambda k, dt: [torch.from_numpy(s[k]).to(device=device, dtype=dt) for s in ss]             # noqa: E731
        ev.update(t("boxes", torch.float32), t("scores", torch.float32), t("labels", torch.int32), valid,
                  g("gt_boxes", torch.float32), g("gt_labels", torch.int64), gt_attrs=g("gt_attrs", torch.int32),
                  gt_num_pts=g("gt_num_pts", torch.int32), pred_attrs=t("attrs", torch.int32),
                  lidar2ego=t("lidar2ego", torch.float64))


def flatten(metrics):
    """metrics_summary layout -> {path: float}"""
    out = {}
    for k, v in metrics.items():
        if isinstance(v, dict):
            for k2, v2 in v.items():
                if isinstance(v2, dict):
                    for k3, v3 in v2.items():
                        out[f"{k}/{k2}/{float(k3) if not isinstance(k3, str) else k3}"] = float(v3)
                else:
                    out[f"{k}/{k2}"] = float(v2)
        else:
            out[k] = float(v)
    return out


def max_metric_error(got, ref):
    """(largest absolute difference over every metric, its path); NaN must meet NaN"""
    a, b = flatten(got), flatten(ref)
    assert set(a) == set(b), set(a) ^ set(b)
    worst, where = 0.0, None
    for k in a:
        if np.isnan(a[k]) or np.isnan(b[k]):
            assert np.isnan(a[k]) and np.isnan(b[k]), (k, a[k], b[k])
            continue
        if abs(a[k] - b[k]) > worst:
            worst, where = abs(a[k] - b[k]), k
    return worst, where
