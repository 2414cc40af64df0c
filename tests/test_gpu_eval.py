"""GPU tests of the detection evaluator (isfusion_amd.evaluation, csrc/isf_eval.hip): compute() against the float64 numpy
restatement of tests/eval_common.py on the same fp32 rows.

Tolerance: both sides are fp64 on identical fp32 inputs and, under the guard (tests/test_eval.py holds it for every
problem here), take identical discrete decisions; what differs is the summation order of the scans and one-ulp libm
differences, over at most 1.3e4 terms of magnitude <= 1e2 -- about 1e-10.  Hence 1e-9 absolute on every metric, and
exact equality on the TP masks and on max_recall_ind."""
import os
import sys

import numpy as np
import pytest
import torch

import eval_common as EC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-9
_REF = {}


def _problem(name):
    """(samples, restatement), computed once and shared"""
    if name not in _REF:
        samples = EC.GPU_PROBLEMS[name]()
        _REF[name] = (samples, EC.evaluate(samples))
    return _REF[name]


def _evaluator():
    from isfusion_amd import evaluation
    return evaluation.NuScenesDetectionEval(EC.CLASSES, config=evaluation.detection_cvpr_2019(), device=DEV)


def _check(ev, samples, ref, what):
    got = ev.compute()
    err, where = EC.max_metric_error(got, ref["metrics"])
    print(f"{what}: max |metric - restatement| = {err:.3e} at {where}; mAP {got['mean_ap']:.6f} NDS {got['nd_score']:.6f}")
    masks = ev.tp_masks().cpu().numpy()
    assert np.array_equal(masks, np.concatenate(ref["tp_masks"])), "TP masks differ from the restatement"
    assert ev.max_recall_ind == ref["max_recall_ind"], (ev.max_recall_ind, ref["max_recall_ind"])
    assert err <= TOL, (err, where)
    return got


def test_small_problem_with_every_special_case():
    samples, ref = _problem("small")
    ev = _evaluator()
    EC.feed(ev, samples, device=DEV)
    m = _check(ev, samples, ref, "small")
    # the special cases are really there
    assert m["label_aps"]["trailer"][4.0] == 0.0 and m["label_aps"]["construction_vehicle"][4.0] == 0.0
    assert m["label_aps"]["motorcycle"][0.5] == 0.0 and m["label_aps"]["motorcycle"][4.0] > 0.0
    assert np.isnan(m["label_tp_errors"]["traffic_cone"]["vel_err"]) and m["label_aps"]["traffic_cone"][0.5] > 0.0
    assert 0.0 < m["label_tp_errors"]["barrier"]["orient_err"] < np.pi / 2 + 1e-6


def test_wide_problem_in_four_updates_equals_one_update_bit_for_bit():
    samples, ref = _problem("wide")
    ev = _evaluator()
    EC.feed(ev, samples, batch=16, device=DEV)
    assert ev.num_samples == 64
    _check(ev, samples, ref, "wide")
    four, curves4 = EC.flatten(ev.compute()), ev.curves().clone()
    one = _evaluator()
    EC.feed(one, samples, device=DEV)
    got = EC.flatten(one.compute())
    assert all(got[k] == four[k] or (np.isnan(got[k]) and np.isnan(four[k])) for k in four)
    assert torch.equal(torch.nan_to_num(one.curves(), nan=-1.0), torch.nan_to_num(curves4, nan=-1.0))
    assert torch.equal(one.tp_masks(), ev.tp_masks())


def test_deep_sample_500_predictions_70_boxes_of_one_class():
    samples, ref = _problem("deep")
    ev = _evaluator()
    EC.feed(ev, samples, counts=True, device=DEV)
    m = _check(ev, samples, ref, "deep")
    assert m["label_aps"]["car"][4.0] > 0.5


def test_ties_follow_the_stated_rule():
    samples, ref = _problem("ties")
    scores = np.concatenate([s["scores"][s["valid"]] for s in samples])
    assert len(np.unique(scores)) <= 6 < len(scores)
    ev = _evaluator()
    EC.feed(ev, samples, batch=2, device=DEV)
    _check(ev, samples, ref, "ties")


def test_negative_scores_are_ordered_not_refused():
    samples, ref = _problem("negative")
    scores = np.concatenate([s["scores"] for s in samples])
    assert (scores < 0).any() and (scores > 0).any()
    ev = _evaluator()
    EC.feed(ev, samples, device=DEV)
    _check(ev, samples, ref, "negative")


@pytest.mark.parametrize("name", ["perfect", "empty", "hand"])
def test_known_answers_on_the_device(name):
    samples, ref = _problem(name)
    ev = _evaluator()
    EC.feed(ev, samples, device=DEV)
    m = _check(ev, samples, ref, name)
    if name == "perfect":
        assert all(abs(ap - 1.0) <= TOL for d in m["label_aps"].values() for ap in d.values())
        assert all(v == 0.0 for v in m["tp_errors"].values())
        assert abs(m["nd_score"] - 1.0) <= TOL
    elif name == "empty":
        assert m["mean_ap"] == 0.0 and m["nd_score"] == 0.0 and all(v == 1.0 for v in m["tp_errors"].values())
    else:
        assert abs(m["label_aps"]["car"][0.5] - 0.4362139918) <= TOL and abs(m["label_aps"]["car"][1.0] - 0.7376543210) <= TOL
        c = ev.curves()[0].cpu().numpy()                       # car: precision x 4, confidence x 4, TP curves x 5
        assert abs(c[0, 50] - 1 / 3) <= TOL and abs(c[4, 50] - np.float32(0.7)) <= TOL and c[0, 49] == 1.0
        assert c[1, 50] == 0.5 and abs(c[5, 50] - np.float32(0.8)) <= TOL
        assert abs(m["label_tp_errors"]["car"]["trans_err"] - 0.36375) < 1e-7      # 0.3 / 10.6 are fp32 roundings
        d = ev.detail()
        assert d["pts_bbox_NuScenes/car_AP_dist_0.5"] == 0.4362 and d["pts_bbox_NuScenes/mAP"] == m["mean_ap"]


def test_update_makes_no_transfer_and_reset_reproduces_the_result():
    samples, ref = _problem("small")
    ev = _evaluator()
    EC.feed(ev, samples, device=DEV)               # warm: library loaded, buffers' first growth
    first = EC.flatten(ev.compute())
    ev.reset()
    assert ev.num_samples == 0
    t = lambda k, dt: torch.from_numpy(np.stack([s[k] for s in samples])).to(device=DEV, dtype=dt)      # noqa: E731
    g = lambda k, dt: [torch.from_numpy(s[k]).to(device=DEV, dtype=dt) for s in samples]                # noqa: E731
    args = (t("boxes", torch.float32), t("scores", torch.float32), t("labels", torch.int32), t("valid", torch.bool),
            g("gt_boxes", torch.float32), g("gt_labels", torch.int64))
    kw = dict(gt_attrs=g("gt_attrs", torch.int32), gt_num_pts=g("gt_num_pts", torch.int32), lidar2ego=t("lidar2ego", torch.float64))
    counts = torch.full((len(samples),), 40, dtype=torch.int32, device=DEV)
    spare = _evaluator()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.update(*args, pred_attrs=None, **kw)    # predicted_attributes on the device
        spare.update(args[0], args[1], args[2], counts, args[4], args[5])      # counts, defaults, a first growth
    finally:
        torch.cuda.set_sync_debug_mode(0)
    again = EC.flatten(ev.compute())
    assert all(again[k] == first[k] or (np.isnan(again[k]) and np.isnan(first[k])) for k in first)
    # the device's attribute heuristic is the restatement's (the problem's attrs were made by it)
    from isfusion_amd import evaluation
    got = evaluation.predicted_attributes(args[2], args[0], EC.CLASSES).cpu().numpy()
    assert np.array_equal(got, np.stack([s["attrs"] for s in samples]))


def test_predicted_attributes_on_both_sides_of_the_speed_limit():
    from isfusion_amd import evaluation
    labels = torch.arange(10, dtype=torch.int32, device=DEV).repeat(2).view(2, 10)
    boxes = torch.zeros(2, 10, 9, device=DEV)
    boxes[0, :, 7], boxes[0, :, 8] = 0.15, 0.15          # 0.212 m/s
    boxes[1, :, 7], boxes[1, :, 8] = 0.14, 0.14          # 0.198 m/s
    got = evaluation.predicted_attributes(labels, boxes, EC.CLASSES).cpu().numpy()
    want = np.array([[EC.predicted_attribute(n, v, v) for n in EC.CLASSES] for v in (0.15, 0.14)])
    assert np.array_equal(got, want)
    out_of_range = evaluation.predicted_attributes(torch.tensor([-1, 10], dtype=torch.int32, device=DEV),
                                                   torch.zeros(2, 9, device=DEV), EC.CLASSES)
    assert out_of_range.tolist() == [-1, -1]


def test_end_to_end_from_decode_and_nms():
    """decode_and_nms outputs of a seeded head fed directly into update; the restatement runs on the copied rows"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_nms as G
    from isfusion_amd.transfusion_head import TransFusionHeadV2
    head = TransFusionHeadV2(test_cfg=dict(dataset="nuScenes", grid_size=[1440, 1440, 40], out_size_factor=8,
                                           nms_type="rotate"), bbox_coder=dict(G.CODER))
    preds, labs = zip(*[G.proposals(s) for s in G.SEEDS])
    pd = {k: torch.cat([p[k] for p in preds]).to(DEV) for k in preds[0]}
    head.query_labels = torch.cat(labs).to(DEV)
    boxes, scores, labels, counts, keep = head.decode_and_nms([[pd]])
    B, P, D = boxes.shape
    assert D == 9 and keep is not None
    hb, hs, hl, hk = boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy(), keep.cpu().numpy()
    rng = np.random.default_rng(EC.E2E_SEED)
    samples, gts = [], []
    for b in range(B):
        rows = np.nonzero(hk[b])[0][::3][:40]                 # every third kept box, moved a little, is a ground truth
        gb = hb[b, rows].copy()
        gb[:, :2] += rng.normal(0, 0.6, (len(rows), 2)).astype(np.float32)
        gb[:, 6] += rng.normal(0, 0.2, len(rows)).astype(np.float32)
        gl = hl[b, rows].astype(np.int32)
        samples.append(EC.make_sample(hb[b], hs[b], hl[b], gb, gl, valid=hk[b], gt_attrs=rng.integers(-1, 8, len(rows))))
        gts.append((torch.from_numpy(gb).to(DEV), torch.from_numpy(gl).to(DEV),
                    torch.from_numpy(samples[-1]["gt_attrs"]).to(DEV)))
    assert EC.guard(samples, allow_ties=True)                 # equal head scores fall under the stated tie rule
    ref = EC.evaluate(samples)
    ev = _evaluator()
    ev.update(boxes, scores, labels, keep, [g[0] for g in gts], [g[1] for g in gts], gt_attrs=[g[2] for g in gts])
    m = _check(ev, samples, ref, "end to end")
    assert m["mean_ap"] > 0.0
