"""CPU tests of the detection evaluator (isfusion_amd.evaluation): the float64 restatement of tests/eval_common.py pinned by
known answers (so that the oracle of tests/test_gpu_eval.py is not its own judge), the attribute table against the
reference's, the evaluator's surface, the C symbols, and the guard of the GPU comparisons for every problem they use."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import eval_common as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL_SYMBOLS = ("isf_eval_attributes", "isf_eval_match", "isf_eval_order", "isf_eval_curves", "isf_eval_scalars")


ONE_ULPS = 1e-12    # "is 1" in float64: AP = mean(90 x (1 - 0.1)) / 0.9 comes out as 1 + 4e-16 by the rounding of the mean


def test_predictions_equal_to_the_ground_truth_score_one():
    """(a) every AP is 1, every error is 0, nd_score is 1 (to float64 rounding, ONE_ULPS)"""
    m = EC.evaluate(EC.perfect_problem())["metrics"]
    for name in EC.CLASSES:
        for th, ap in m["label_aps"][name].items():
            assert abs(ap - 1.0) < ONE_ULPS, (name, th, ap)
        for k, v in m["label_tp_errors"][name].items():
            assert v == 0.0 or np.isnan(v), (name, k, v)
    assert np.isnan(m["label_tp_errors"]["traffic_cone"]["orient_err"]) and m["label_tp_errors"]["barrier"]["orient_err"] == 0.0
    assert all(v == 0.0 for v in m["tp_errors"].values()), m["tp_errors"]
    assert abs(m["mean_ap"] - 1.0) < ONE_ULPS and abs(m["nd_score"] - 1.0) < ONE_ULPS


def test_no_valid_prediction_scores_zero():
    """(b) mean_ap == 0, errors are 1, nd_score == 0"""
    r = EC.evaluate(EC.empty_problem())
    m = r["metrics"]
    assert m["mean_ap"] == 0.0 and m["nd_score"] == 0.0
    assert all(v == 1.0 for v in m["tp_errors"].values()), m["tp_errors"]
    for name in EC.CLASSES:
        assert all(v == 1.0 or np.isnan(v) for v in m["label_tp_errors"][name].values())
        assert r["max_recall_ind"][name] == 0
    assert all(not mask.any() for mask in r["tp_masks"])


def test_hand_case():
    """(c) one class, npos = 2, predictions (0.9, 0.3 m), (0.8, no box within 4 m), (0.7, 0.6 m to the other box).  The
    coordinates are fp32 roundings of 0.3 / 10.6, hence 1e-7 on the values that depend on them."""
    r = EC.evaluate(EC.hand_problem())
    m, car = r["metrics"], r["curves"]["car"]
    assert [int(x) for x in r["tp_masks"][0]] == [0b1111, 0, 0b1110]
    assert abs(m["label_aps"]["car"][0.5] - 0.4362139918) < 1e-9
    assert abs(car[0.5]["precision"][50] - 1 / 3) < 1e-12 and abs(car[0.5]["confidence"][50] - np.float32(0.7)) < 1e-12
    assert car[0.5]["precision"][49] == 1.0
    assert abs(m["label_aps"]["car"][1.0] - 0.7376543210) < 1e-9
    # the last-of-duplicates rule: rec = [0.5, 0.5, 1.0]; x = 0.5 reads row 1
    assert car[1.0]["precision"][50] == 0.5 and abs(car[1.0]["confidence"][50] - np.float32(0.8)) < 1e-12
    assert abs(m["label_tp_errors"]["car"]["trans_err"] - 0.36375) < 1e-7
    assert r["max_recall_ind"]["car"] == 100
    for name in EC.CLASSES[1:]:
        assert m["mean_dist_aps"][name] == 0.0


def _reference_attribute(name, speed_over):
    """nuscenes_dataset.py:378-397 over the tables of :70-91, read off the reference by hand"""
    moving = {"car": "vehicle.moving", "construction_vehicle": "vehicle.moving", "bus": "vehicle.moving",
              "truck": "vehicle.moving", "trailer": "vehicle.moving", "bicycle": "cycle.with_rider",
              "motorcycle": "cycle.with_rider", "pedestrian": "pedestrian.moving", "barrier": "", "traffic_cone": ""}
    still = {"car": "vehicle.parked", "construction_vehicle": "vehicle.parked", "bus": "vehicle.stopped",
             "truck": "vehicle.parked", "trailer": "vehicle.parked", "bicycle": "cycle.without_rider",
             "motorcycle": "cycle.without_rider", "pedestrian": "pedestrian.standing", "barrier": "", "traffic_cone": ""}
    ids = ["cycle.with_rider", "cycle.without_rider", "pedestrian.moving", "pedestrian.standing",
           "pedestrian.sitting_lying_down", "vehicle.moving", "vehicle.parked", "vehicle.stopped"]
    a = (moving if speed_over else still)[name]
    return ids.index(a) if a else -1


def test_attribute_table_matches_the_reference():
    """(d) every class on both sides of 0.2 m/s: the module's host tables and the restatement's per-box function"""
    from isfusion_amd import evaluation
    moving, still = evaluation.attribute_tables(EC.CLASSES)
    for c, name in enumerate(EC.CLASSES):
        assert moving[c] == _reference_attribute(name, True) == EC.predicted_attribute(name, 0.15, 0.15), name
        assert still[c] == _reference_attribute(name, False) == EC.predicted_attribute(name, 0.14, 0.14), name
    assert evaluation.ATTR_MAPPING == EC.ATTR_MAPPING and evaluation.DEFAULT_ATTRIBUTE == EC.DEFAULT_ATTRIBUTE
    assert evaluation.CLASSES == EC.CLASSES


def test_config_and_detail_key_set():
    """(e) detection_cvpr_2019 and detail()'s keys for the shipped ten class names"""
    from isfusion_amd import evaluation
    cfg = evaluation.detection_cvpr_2019()
    assert cfg == EC.CONFIG
    ev = evaluation.NuScenesDetectionEval(EC.CLASSES, config=cfg)          # touches no device
    ref = EC.evaluate(EC.hand_problem())["metrics"]
    ev._metrics = {**ref, "label_aps": {n: {float(k): v for k, v in d.items()} for n, d in ref["label_aps"].items()}}
    d = ev.detail(result_name="pts_bbox")
    want = {"pts_bbox_NuScenes/NDS", "pts_bbox_NuScenes/mAP"}
    want |= {f"pts_bbox_NuScenes/{n}" for n in ("mATE", "mASE", "mAOE", "mAVE", "mAAE")}
    for name in EC.CLASSES:
        want |= {f"pts_bbox_NuScenes/{name}_AP_dist_{t}" for t in ("0.5", "1.0", "2.0", "4.0")}
        want |= {f"pts_bbox_NuScenes/{name}_{m}" for m in EC.TP_METRICS}
    assert set(d) == want
    assert d["pts_bbox_NuScenes/car_AP_dist_0.5"] == 0.4362 and d["pts_bbox_NuScenes/car_trans_err"] == 0.3638
    assert d["pts_bbox_NuScenes/mAP"] == ref["mean_ap"] and d["pts_bbox_NuScenes/NDS"] == ref["nd_score"]


def test_eval_symbols_declared_mirrored_and_exported():
    from isfusion_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "isf_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in EVAL_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(_lib.SIGNATURES["isf_eval_match"][1]) == 29 and len(_lib.SIGNATURES["isf_eval_curves"][1]) == 12


def test_update_refuses_cpu_tensors_and_oversized_samples():
    from isfusion_amd import evaluation
    from isfusion_amd._lib import IsfError
    ev = evaluation.NuScenesDetectionEval(EC.CLASSES)
    b, s, lab = torch.zeros(1, 4, 9), torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.int32)
    with pytest.raises(IsfError, match="GPU"):
        ev.update(b, s, lab, torch.ones(1, 4, dtype=torch.bool), [torch.zeros(2, 9)], [torch.zeros(2, dtype=torch.int64)])
    with pytest.raises(IsfError):
        evaluation.predicted_attributes(lab, b, EC.CLASSES)
    with pytest.raises(IsfError, match="500"):           # the shape checks come before any device work
        ev.update(torch.zeros(1, 501, 9), torch.zeros(1, 501), torch.zeros(1, 501, dtype=torch.int32), None,
                  [torch.zeros(0, 9)], [torch.zeros(0)])
    with pytest.raises(IsfError, match="1024"):
        ev.update(b, s, lab, None, [torch.zeros(1025, 9)], [torch.zeros(1025)])
    assert ev.num_samples == 0


@pytest.mark.parametrize("name", sorted(EC.GPU_PROBLEMS))
def test_guard_holds_for_every_gpu_problem(name):
    """(f)"""
    assert EC.guard(EC.GPU_PROBLEMS[name](), allow_ties=(name == "ties"))


def test_guard_refuses_a_threshold_a_range_and_a_duplicate_score():
    """the guard is not vacuous: each of its three conditions fails on a problem built to break it (the end-to-end GPU
    case, whose rows only exist on the device, runs the guard on the copied rows itself)"""
    s = EC.hand_problem()
    s[0]["boxes"][0, 0] = np.float32(0.5)                   # exactly on the 0.5 m threshold
    with pytest.raises(AssertionError, match="threshold"):
        EC.guard(s)
    s = EC.hand_problem()
    s[0]["scores"][1] = s[0]["scores"][0]
    with pytest.raises(AssertionError, match="duplicate"):
        EC.guard(s)
    s = EC.hand_problem()
    s[0]["gt_boxes"][1, :2] = (50.0, 0.0)                   # exactly on the car range
    with pytest.raises(AssertionError, match="range"):
        EC.guard(s)
