"""CPU tests of the detection head's training surface: the restated third-party pieces of
tests/golden/make_golden_head_loss.py reproduce the reference's golden values, the head takes the reference's training
configuration (registry build of the unmodified config carries train_cfg; unsupported loss types raise)."""
import ast
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_head_loss as G  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "head_loss_ref.npz"), allow_pickle=False)


@pytest.mark.parametrize("name", list(G.CASES))
def test_restated_losses_reproduce_the_golden(name):
    gts, pd = G.head_loss_case(name)
    hm = torch.from_numpy(GOLD[f"{name}.heatmap"])
    avg = max(float(hm.eq(1).sum()), 1.0)
    clip = lambda t: t.sigmoid().clamp(1e-4, 1 - 1e-4)
    for key, src in (("loss_heatmap", "dense_heatmap"), ("loss_heatmap_ins", "ins_heatmap")):
        got = float(G.gaussian_focal_loss(clip(pd[src]), hm, avg))
        assert abs(got - float(GOLD[f"{name}.loss.{key}"])) <= 1e-9 * abs(got), key
    npos = max(int(GOLD[f"{name}.num_pos"]), 1)
    labels = torch.from_numpy(GOLD[f"{name}.labels"]).reshape(-1)
    lw = torch.from_numpy(GOLD[f"{name}.label_weights"]).reshape(-1)
    cls = G.sigmoid_focal_loss(pd["heatmap"].permute(0, 2, 1).reshape(-1, G.C), labels, lw, avg_factor=npos)
    assert abs(float(cls) - float(GOLD[f"{name}.loss.layer_-1_loss_cls"])) <= 1e-9 * abs(float(cls))
    preds = torch.cat([pd[k] for k in ("center", "height", "dim", "rot", "vel")], 1).permute(0, 2, 1)
    w = torch.from_numpy(GOLD[f"{name}.bbox_weights"]).double() * torch.tensor(G.TRAIN_CFG["code_weights"]).double()
    bbox = G.l1_loss(preds, torch.from_numpy(GOLD[f"{name}.bbox_targets"]), w, npos, 0.25)
    assert abs(float(bbox) - float(GOLD[f"{name}.loss.layer_-1_loss_bbox"])) <= 1e-9 * abs(float(bbox))


def test_restated_iou_and_cost_reproduce_the_golden():
    gts, pd = G.head_loss_case("g40_150")
    for b in range(G.B):
        boxes = torch.from_numpy(GOLD[f"g40_150.{b}.pred_boxes"])
        gt, lab = gts[b]
        iou = G.iou3d(boxes, gt)
        assert (iou - torch.from_numpy(GOLD[f"g40_150.{b}.iou"]).double()).abs().max().item() <= 1e-5
        cls = G.focal_loss_cost(pd["heatmap"][b].T, lab)
        pcr = torch.tensor(G.TRAIN_CFG["point_cloud_range"], dtype=torch.float64)
        norm = lambda t: (t[:, :2].double() - pcr[:2]) / (pcr[3:5] - pcr[:2])
        reg = torch.cdist(norm(boxes), norm(gt), p=1) * 0.25
        cost = cls + reg - 0.25 * iou
        assert (cost - torch.from_numpy(GOLD[f"g40_150.{b}.cost"]).double()).abs().max().item() <= 1e-5


def test_scipy_assignment_of_the_golden_cost_is_the_golden_assignment():
    scipy_opt = pytest.importorskip("scipy.optimize")
    for b in range(G.B):
        cost = GOLD[f"g40_150.{b}.cost"].astype(np.float64)
        rows, cols = scipy_opt.linear_sum_assignment(cost)
        want = np.zeros(cost.shape[0], np.int64)
        want[rows] = cols + 1
        assert np.array_equal(want, GOLD[f"g40_150.{b}.assigned_gt_inds"])


def test_head_takes_the_training_configuration():
    from isfusion_amd.transfusion_head import TransFusionHeadV2
    h = TransFusionHeadV2(train_cfg=G.TRAIN_CFG)
    assert h.train_cfg["min_radius"] == 2 and h.loss_cls["type"] == "FocalLoss" and h.loss_bbox["loss_weight"] == 0.25
    assert callable(h.loss) and callable(h.get_targets)
    with pytest.raises(NotImplementedError, match="SmoothL1Loss"):
        TransFusionHeadV2(loss_bbox=dict(type="SmoothL1Loss"))
    with pytest.raises(NotImplementedError, match="HeuristicAssigner"):
        TransFusionHeadV2(train_cfg=dict(G.TRAIN_CFG, assigner=dict(type="HeuristicAssigner")))
    with pytest.raises(RuntimeError, match="train_cfg"):
        TransFusionHeadV2().get_targets([], [], [{"heatmap": torch.zeros(1, 10, 200)}])


def test_registry_build_carries_train_cfg():
    from isfusion_amd import registry
    from isfusion_amd.detector import ISFusionPtsPath
    with open(os.path.join(ROOT, "tests", "golden", "isfusion_0075voxel_model.txt")) as f:
        model = ast.literal_eval(f.read())
    net = registry.build_pts_path({"model": model})
    head = net.pts_bbox_head
    assert head.train_cfg == dict(model["train_cfg"]["pts"])
    assert head.train_cfg["assigner"]["type"] == "HungarianAssigner3D" and head.train_cfg["code_weights"][-1] == 0.2
    assert head.loss_heatmap["type"] == "GaussianFocalLoss" and head.loss_cls["alpha"] == 0.25
    ref = ISFusionPtsPath()
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == \
        {k: tuple(v.shape) for k, v in ref.state_dict().items()}
