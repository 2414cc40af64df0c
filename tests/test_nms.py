"""CPU tests of the NMS / test-time-augmentation surface: the restated pieces of tests/golden/make_golden_nms.py
reproduce the reference's golden values, flip_tta_views matches RandomFlip3DV2's test branch, and the head's
configuration accepts nms_type 'circle' / 'rotate' (unknown types still raise)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_nms as G  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "nms_ref.npz"), allow_pickle=False)


@pytest.mark.parametrize("name", ["one", "cut"])
def test_restated_nms_reproduces_the_golden(name):
    case = G.edge_cases()[name]
    xyxyr, s, b = case
    assert np.array_equal(xyxyr.numpy(), GOLD[f"edge.{name}.xyxyr"])
    assert np.array_equal(G.nms_gpu(xyxyr, s, 0.1).numpy(), GOLD[f"edge.{name}.rotate"])
    assert np.array_equal(G.nms_gpu(xyxyr, s, 0.1, pre_maxsize=20, post_max_size=5).numpy(),
                          GOLD[f"edge.{name}.rotate_cut"])
    assert np.array_equal(G.nms_normal_gpu(xyxyr, s, 0.1).numpy(), GOLD[f"edge.{name}.normal"])
    dets = torch.cat([b[:, :2], s[:, None]], 1).numpy()
    assert G.circle_nms_restated(dets, 0.5, post_max_size=5) == list(GOLD[f"edge.{name}.circle"])


def test_cut_case_suppresses_and_cuts():
    assert len(GOLD["edge.cut.rotate"]) < len(GOLD["edge.cut.scores"])
    assert len(GOLD["edge.cut.rotate_cut"]) == 5
    assert len(GOLD["edge.cut.circle"]) == 5


def test_restated_circle_nms_matches_the_reference():
    assert G.circle_nms_restated(GOLD["circle.dets"], 0.175) == list(GOLD["circle.keep"])


def test_golden_get_bboxes_suppresses_only_pedestrian_and_cone():
    for nms_type in ("circle", "rotate"):
        for seed in G.SEEDS:
            preds, qlab = G.proposals(seed)
            labels = GOLD[f"get_bboxes.{nms_type}.{seed}.labels"]
            n_in = np.bincount(qlab[0, :120].numpy(), minlength=10)
            n_out = np.bincount(labels, minlength=10)
            assert np.array_equal(n_in[:8], n_out[:8])            # radius -1: passed through
            assert (n_out[8:] < n_in[8:]).all()                   # NMS'd


def test_restated_mapping_back_matches_the_reference():
    for seed in G.SEEDS:
        for v, (h, vf) in enumerate(G.VIEW_FLIPS):
            b = torch.from_numpy(GOLD[f"tta.v4.{seed}.{v}.boxes"])
            assert np.allclose(G.mapping_back_restated(b, 1.0, h, vf).numpy(), GOLD[f"tta.v4.{seed}.{v}.mapped"],
                               atol=0, rtol=0)
        for v in range(2):
            b = torch.from_numpy(GOLD[f"tta.v2s.{seed}.{v}.boxes"])
            got = G.mapping_back_restated(b, 1.25, *G.VIEW_FLIPS[v]).numpy()
            assert np.allclose(got, GOLD[f"tta.v2s.{seed}.{v}.mapped"], rtol=1e-6, atol=1e-6)


def test_flip_tta_views_matches_random_flip_3d_v2():
    from isfusion_amd.input_pipeline import flip_tta_views
    pts, lam = GOLD["flip.points"], GOLD["flip.lam"]
    vp, vm = flip_tta_views(pts, dict(lidar_aug_matrix=lam), flip=True, pcd_horizontal_flip=True,
                            pcd_vertical_flip=True)
    assert [(m["pcd_horizontal_flip"], m["pcd_vertical_flip"]) for m in vm] == G.VIEW_FLIPS
    for p, m, (h, vf) in zip(vp, vm, G.VIEW_FLIPS):
        key = f"flip.{int(h)}{int(vf)}"
        assert np.array_equal(p, GOLD[key + ".points"])
        assert np.array_equal(m["lidar_aug_matrix"], GOLD[key + ".lam"])
        assert m["pcd_scale_factor"] == 1.0
        assert m["transformation_3d_flow"] == (["HF"] if h else []) + (["VF"] if vf else [])
    tp, _ = flip_tta_views(torch.from_numpy(pts), dict(lidar_aug_matrix=lam))
    assert np.array_equal(tp[3].numpy(), GOLD["flip.11.points"])
    # MultiScaleFlipAug3D's enumeration: no flip -> one view per scale; flips only with `flip`
    assert len(flip_tta_views(pts, {}, flip=False)[0]) == 1
    assert len(flip_tta_views(pts, {}, pcd_vertical_flip=False)[0]) == 2
    _, ms = flip_tta_views(pts, {}, pcd_horizontal_flip=False, pcd_vertical_flip=False, pts_scale_ratio=(1.0, 1.25))
    assert [m["pcd_scale_factor"] for m in ms] == [1.0, 1.25]


def test_head_accepts_circle_and_rotate_and_rejects_unknown_nms_types():
    from isfusion_amd.transfusion_head import TransFusionHeadV2
    cfg = dict(dataset="nuScenes", grid_size=[64, 64, 40], out_size_factor=8)
    for t in ("circle", "rotate"):
        plan = TransFusionHeadV2(test_cfg=dict(cfg, nms_type=t))._nms_plan()
        assert plan["modes"] == ["keep", t, t] and plan["thresholds"] == [-1.0, 0.175, 0.175]
        assert plan["task_of_class"] == [0] * 8 + [1, 2]
        assert plan["post_max_size"] == (83 if t == "circle" else None)
    assert TransFusionHeadV2(test_cfg=dict(cfg, nms_type=None))._nms_plan() is None
    assert TransFusionHeadV2(test_cfg=cfg)._nms_plan() is None
    with pytest.raises(NotImplementedError):
        TransFusionHeadV2(test_cfg=dict(cfg, nms_type="weighted"))._nms_plan()
    waymo = TransFusionHeadV2(num_classes=3, test_cfg=dict(cfg, dataset="Waymo", nms_type="rotate",
                                                           pre_maxsize=100, post_maxsize=50))._nms_plan()
    assert waymo["modes"] == ["rotate"] * 3 and waymo["pre_maxsize"] == 100 and waymo["post_max_size"] == 50


def test_nms_entry_points_exist_and_refuse_cpu_tensors():
    from isfusion_amd import _lib, nms
    for name in ("boxes_iou_bev", "nms_gpu", "nms_normal_gpu", "circle_nms", "xywhr2xyxyr", "segmented_nms",
                 "merge_aug_bboxes_3d", "bbox3d_mapping_back"):
        assert callable(getattr(nms, name))
    with pytest.raises(_lib.IsfError):
        nms.nms_gpu(torch.zeros((3, 5)), torch.zeros(3), 0.1)
    with pytest.raises(_lib.IsfError):
        nms.segmented_nms(torch.zeros((2048, 7)), torch.zeros(2048), ["rotate"], [0.1], 2048)
    with pytest.raises(NotImplementedError):
        nms.merge_aug_bboxes_3d([], [], {}, weighted_nms=True)
    x = torch.tensor([[1.0, 2.0, 4.0, 2.0, 0.3]])
    assert torch.equal(nms.xywhr2xyxyr(x), torch.tensor([[-1.0, 1.0, 3.0, 3.0, 0.3]]))


def test_detector_has_the_test_time_entry_points():
    from isfusion_amd.detector import ISFusionPtsPath
    for name in ("aug_test", "aug_test_pts", "forward_test", "simple_test"):
        assert callable(getattr(ISFusionPtsPath, name))
