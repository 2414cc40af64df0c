"""GPU tests of the BEV NMS and test-time augmentation (isf_nms.hip through isfusion_amd.nms, TransFusionHeadV2.
get_bboxes with nms_type 'circle' / 'rotate', ISFusionPtsPath.aug_test) against the reference's own results
(tests/golden/nms_ref.npz, tests/golden/make_golden_nms.py) and float64 restatements."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_nms as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = np.load(os.path.join(HERE, "golden", "nms_ref.npz"), allow_pickle=False)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_boxes_iou_bev_equals_the_float64_restatement():
    from isfusion_amd import nms
    x = _t(GOLD["edge.cut.xyxyr"])
    got = nms.boxes_iou_bev(x, x).cpu().numpy()
    assert np.abs(got - GOLD["edge.cut.iou"]).max() < 1e-5
    assert got.shape == (30, 30) and (np.diag(got) > 0.999).all()
    assert nms.boxes_iou_bev(x[:0], x).shape == (0, 30)


@pytest.mark.parametrize("name", ["one", "cut"])
def test_each_mode_equals_the_golden(name):
    from isfusion_amd import nms
    x, s, b = _t(GOLD[f"edge.{name}.xyxyr"]), _t(GOLD[f"edge.{name}.scores"]), _t(GOLD[f"edge.{name}.lidar"])
    assert np.array_equal(nms.nms_gpu(x, s, 0.1).cpu().numpy(), GOLD[f"edge.{name}.rotate"])
    assert np.array_equal(nms.nms_gpu(x, s, 0.1, pre_maxsize=20, post_max_size=5).cpu().numpy(),
                          GOLD[f"edge.{name}.rotate_cut"])
    assert np.array_equal(nms.nms_normal_gpu(x, s, 0.1).cpu().numpy(), GOLD[f"edge.{name}.normal"])
    dets = torch.cat([b[:, :2], s[:, None]], 1)
    assert np.array_equal(nms.circle_nms(dets, 0.5, post_max_size=5).cpu().numpy(), GOLD[f"edge.{name}.circle"])
    # the LiDAR-row layout gives the same rotate result as its xywhr2xyxyr
    _, idx, cnt = nms.segmented_nms(b, s, ["rotate"], [0.1], b.shape[0], box_format=nms.BOX_LIDAR)
    assert np.array_equal(idx[0, :int(cnt[0])].cpu().numpy(), GOLD[f"edge.{name}.rotate"])


def test_circle_nms_equals_the_reference():
    from isfusion_amd import nms
    got = nms.circle_nms(_t(GOLD["circle.dets"]), 0.175)
    assert np.array_equal(got.cpu().numpy(), GOLD["circle.keep"])


def test_segments_never_suppress_each_other():
    from isfusion_amd import nms
    b, s = _t(GOLD["edge.cut.lidar"]), _t(GOLD["edge.cut.scores"])
    n = b.shape[0]
    # three groups of the same boxes (counts 30, 12, 0), labels split over two tasks
    bb, ss = b.repeat(3, 1), s.repeat(3)
    lab = torch.tensor([0, 1] * (n // 2), dtype=torch.int32, device=DEV).repeat(3)
    counts = torch.tensor([n, 12, 0], dtype=torch.int32, device=DEV)
    keep, idx, cnt = nms.segmented_nms(bb, ss, ["rotate", "circle"], [0.1, 0.5], n, labels=lab, counts=counts,
                                       task_of_class=[0, 1])
    for g, c in enumerate([n, 12, 0]):
        for t, (mode, thr) in enumerate([("rotate", 0.1), ("circle", 0.5)]):
            rows = [r for r in range(c) if r % 2 == t]
            if rows:
                _, ref, rc = nms.segmented_nms(b[rows], s[rows], [mode], [thr], len(rows))
                want = [rows[i] + g * n for i in ref[0, :int(rc[0])].cpu().tolist()]
            else:
                want = []
            k = int(cnt[g * 2 + t])
            assert idx[g * 2 + t, :k].cpu().tolist() == want, (g, t)
        assert not keep[g * n + c:(g + 1) * n].any()


def test_empty_single_and_full_segments():
    from isfusion_amd import nms
    z = torch.zeros((0, 5), device=DEV)
    assert nms.nms_gpu(z, torch.zeros(0, device=DEV), 0.1).numel() == 0
    assert nms.circle_nms(torch.zeros((0, 3), device=DEV), 0.1).numel() == 0
    one = _t(GOLD["edge.one.xyxyr"])
    assert nms.nms_gpu(one, _t(GOLD["edge.one.scores"]), 0.1).cpu().tolist() == [0]
    g = torch.Generator().manual_seed(1)
    xy = torch.rand((1024, 2), generator=g, dtype=torch.float64) * 20
    sc = torch.randperm(1024, generator=g).double() / 1024 + 0.001
    dets = torch.cat([xy, sc[:, None]], 1)
    want = G.circle_nms_restated(dets.numpy(), 0.5, post_max_size=2000)
    got = nms.circle_nms(dets.float().to(DEV), 0.5, post_max_size=None)
    assert got.cpu().tolist() == want
    wh = torch.rand((1024, 2), generator=g) * 2 + 0.5
    x = torch.cat([xy.float() - wh / 2, xy.float() + wh / 2, torch.zeros((1024, 1))], 1)
    want = G.nms_normal_gpu(x, sc.float(), 0.3).tolist()
    assert nms.nms_normal_gpu(x.to(DEV), sc.float().to(DEV), 0.3).cpu().tolist() == want


def test_more_than_1024_boxes_raise_before_any_launch():
    from isfusion_amd import _lib, nms
    b = torch.zeros((1025, 5), device=DEV)
    with pytest.raises(_lib.IsfError, match="at most 1024"):
        nms.nms_gpu(b, torch.zeros(1025, device=DEV), 0.1)


def _head(nms_type):
    from isfusion_amd.transfusion_head import TransFusionHeadV2
    head = TransFusionHeadV2(test_cfg=dict(dataset="nuScenes", grid_size=[1440, 1440, 40], out_size_factor=8,
                                           nms_type=nms_type), bbox_coder=dict(G.CODER))
    return head


def _batched_preds():
    preds, labs = zip(*[G.proposals(s) for s in G.SEEDS])
    pd = {k: torch.cat([p[k] for p in preds]).to(DEV) for k in preds[0]}
    return [[pd]], torch.cat(labs).to(DEV)


@pytest.mark.parametrize("nms_type", ["circle", "rotate"])
def test_get_bboxes_equals_the_golden(nms_type):
    head = _head(nms_type)
    preds, head.query_labels = _batched_preds()
    res = head.get_bboxes(preds)
    for i, seed in enumerate(G.SEEDS):
        key = f"get_bboxes.{nms_type}.{seed}"
        b, s, lab = res[i]
        assert np.array_equal(lab.cpu().numpy(), GOLD[key + ".labels"])
        assert np.abs(b.cpu().numpy() - GOLD[key + ".boxes"]).max() < 1e-5 * 60
        assert np.abs(s.cpu().numpy() - GOLD[key + ".scores"]).max() < 1e-5


def test_nms_type_none_is_bit_identical_to_decode_boxes():
    from isfusion_amd import fusion_ops as ops
    head = _head(None)
    preds, head.query_labels = _batched_preds()
    res = head.get_bboxes(preds)
    pd, bc = preds[0][0], head.bbox_coder
    cell = [bc["out_size_factor"] * bc["voxel_size"][0], bc["out_size_factor"] * bc["voxel_size"][1]]
    boxes, scores, labels, counts = ops.decode_boxes(pd["heatmap"], pd["query_heatmap_score"], head.query_labels,
                                                     pd["center"], pd["height"], pd["dim"], pd["rot"], pd["vel"], cell,
                                                     bc["pc_range"], bc["post_center_range"], bc["score_threshold"])
    for i, n in enumerate(counts.tolist()):
        assert torch.equal(res[i][0], boxes[i, :n]) and torch.equal(res[i][1], scores[i, :n])
        assert torch.equal(res[i][2], labels[i, :n])


def _merge_restated(views, metas, cfg):
    """merge_aug_bboxes_3d with make_golden_nms's restated nms_gpu / nms_normal_gpu, in float64"""
    bs = [G.mapping_back_restated(b.double().cpu(), m["pcd_scale_factor"], m["pcd_horizontal_flip"],
                                  m["pcd_vertical_flip"]) for (b, _, _), m in zip(views, metas)]
    boxes, scores = torch.cat(bs), torch.cat([s.double().cpu() for _, s, _ in views])
    labels = torch.cat([lab.long().cpu() for _, _, lab in views])
    if boxes.shape[0] == 0:
        return boxes, scores, labels
    x = G.xyxyr_of(boxes.float())
    fn = G.nms_gpu if cfg["use_rotate_nms"] else G.nms_normal_gpu
    mb, ms, ml = [], [], []
    for c in range(int(labels.max()) + 1):
        m = torch.nonzero(labels == c)[:, 0]
        if len(m) == 0:
            continue
        sel = m[fn(x[m], scores[m], cfg["nms_thr"])]
        mb.append(boxes[sel]), ms.append(scores[sel]), ml.append(labels[sel])
    mb, ms, ml = torch.cat(mb), torch.cat(ms), torch.cat(ml)
    order = torch.sort(ms, descending=True, stable=True).indices[:min(cfg["max_num"], boxes.shape[0])]
    return mb[order], ms[order], ml[order]


@pytest.mark.parametrize("rot", [True, False])
@pytest.mark.parametrize("tag", ["v4", "v2s"])
def test_tta_merge_equals_the_golden(tag, rot):
    from isfusion_amd import nms
    nv, scale = (4, 1.0) if tag == "v4" else (2, 1.25)
    for seed in G.SEEDS:
        res, metas = [], []
        for v in range(nv):
            k = f"tta.{tag}.{seed}.{v}"
            res.append(dict(boxes_3d=_t(GOLD[k + ".boxes"]), scores_3d=_t(GOLD[k + ".scores"]),
                            labels_3d=_t(GOLD[k + ".labels"])))
            h, vf = G.VIEW_FLIPS[v]
            metas.append([dict(pcd_scale_factor=scale, pcd_horizontal_flip=h, pcd_vertical_flip=vf)])
            mapped = nms.bbox3d_mapping_back(res[-1]["boxes_3d"], scale, h, vf)
            assert np.abs(mapped.cpu().numpy() - GOLD[k + ".mapped"]).max() < 1e-5
        cfg = dict(G.TTA_CFG, use_rotate_nms=rot)
        torch.cuda.synchronize()
        out = nms.merge_aug_bboxes_3d(res, metas, cfg)
        key = f"tta.{tag}.{seed}.{'rotate' if rot else 'normal'}"
        assert np.array_equal(out["labels_3d"].cpu().numpy(), GOLD[key + ".labels"])
        assert np.abs(out["scores_3d"].cpu().numpy() - GOLD[key + ".scores"]).max() < 1e-6
        assert np.abs(out["boxes_3d"].cpu().numpy() - GOLD[key + ".boxes"]).max() < 1e-4


# ------------------------------------------------------------------------------------------------- detector TTA
_NET = {}


def _detector():
    if "net" not in _NET:
        from detector_common import build_path, detector_inputs
        net = build_path().to(DEV).eval()
        net.pts_bbox_head.test_cfg = dict(net.pts_bbox_head.test_cfg, **G.TTA_CFG)
        pts, inp, kw, metas = detector_inputs()
        _NET["net"] = net
        _NET["frame"] = (pts[0], inp, kw, metas[0])
    return _NET["net"], _NET["frame"]


def _views(n_views, flips=True):
    from isfusion_amd.input_pipeline import flip_tta_views
    net, (p, inp, kw, meta) = _detector()
    m = dict(meta, lidar_aug_matrix=kw["lidar_aug_matrix"][0].numpy())
    if flips:
        vp, vm = flip_tta_views(p, m, pcd_vertical_flip=n_views == 4)
    else:
        vp, vm = flip_tta_views(p, m, flip=False, pts_scale_ratio=(1.0,) * n_views)
    assert len(vp) == n_views
    img = tuple(torch.from_numpy(a[:6]).to(DEV) for a in inp["img_feats"])       # the frame's six cameras
    args = dict(lidar2img=kw["lidar2img"][:1], img_aug_matrix=kw["img_aug_matrix"][:1])
    return net, [torch.from_numpy(x).to(DEV) for x in vp], vm, img, args


def _per_view(net, pts, metas, img, args):
    """the batched forward + per-view get_bboxes of aug_test, for the restated merge"""
    V = len(pts)
    lam = torch.stack([torch.as_tensor(m["lidar_aug_matrix"]) for m in metas])
    feats = tuple(f.repeat(V, 1, 1, 1) for f in img)
    x = net.pts_neck(net.extract_pts_feat(pts, feats, metas, lidar2img=args["lidar2img"].expand(V, -1, -1, -1),
                                          img_aug_matrix=args["img_aug_matrix"].expand(V, -1, -1, -1),
                                          lidar_aug_matrix=lam))
    return net.pts_bbox_head.get_bboxes(net.pts_bbox_head(x, feats, metas), metas)


@pytest.mark.parametrize("n_views", [2, 4])
def test_aug_test_merge_equals_the_restatement(n_views):
    net, pts, metas, img, args = _views(n_views)
    out = net.aug_test(pts, metas, img, **args)
    assert len(out) == 1 and set(out[0]["pts_bbox"]) == {"boxes_3d", "scores_3d", "labels_3d"}
    got = out[0]["pts_bbox"]
    per_view = _per_view(net, pts, metas, img, args)
    assert len(per_view) == n_views
    for b, s, lab in per_view:
        assert b.shape[0] <= net.pts_bbox_head.num_proposals
    want = _merge_restated(per_view, metas, net.pts_bbox_head.test_cfg)
    assert got["boxes_3d"].shape[0] == want[0].shape[0] > 0
    assert np.array_equal(got["labels_3d"].cpu().numpy(), want[2].numpy())
    assert np.abs(got["scores_3d"].cpu().double().numpy() - want[1].numpy()).max() < 1e-6
    assert np.abs(got["boxes_3d"].cpu().double().numpy() - want[0].numpy()).max() < 1e-4
    # forward_test dispatches several augmentations to aug_test
    ft = net.forward_test([[p] for p in pts], [[m] for m in metas], img, **args)
    assert torch.equal(ft[0]["pts_bbox"]["boxes_3d"], got["boxes_3d"])


def test_aug_test_of_unflipped_views_matches_simple_test():
    net, pts, metas, img, args = _views(2, flips=False)
    got = net.aug_test(pts, metas, img, **args)[0]["pts_bbox"]
    lam = torch.as_tensor(metas[0]["lidar_aug_matrix"])[None]
    ref = net.simple_test(pts[:1], metas[:1], img, lidar_aug_matrix=lam, **args)[0]["pts_bbox"]
    rb = ref["boxes_3d"].to(DEV)
    assert got["boxes_3d"].shape[0] > 0
    for b, lab in zip(got["boxes_3d"], got["labels_3d"]):
        d = (rb - b[None]).abs().max(1).values
        d = torch.where(ref["labels_3d"].to(DEV) == lab, d, torch.full_like(d, 1e9))
        assert float(d.min()) < 1e-4


def test_flipped_views_sample_the_unflipped_pixels():
    from isfusion_amd import fusion_ops as ops
    net, pts, metas, img, args = _views(4)
    lam = torch.stack([torch.as_tensor(m["lidar_aug_matrix"]) for m in metas])
    cam = ops.p2g_camera_params(args["lidar2img"].expand(4, -1, -1, -1), args["img_aug_matrix"].expand(4, -1, -1, -1),
                                lam).double().view(4, 6, 20)
    p0 = pts[0][:, :3].double().cpu()
    for v in range(1, 4):
        pv = pts[v][:, :3].double().cpu()
        for c in range(6):
            m0, m1 = cam[0, c, :9].view(3, 3), cam[v, c, :9].view(3, 3)
            a = p0 @ m0.T + cam[0, c, 9:12]
            b = pv @ m1.T + cam[v, c, 9:12]
            assert (a - b).abs().max() < 1e-3 * max(1.0, float(a.abs().max()))


def test_nms_and_merge_make_no_host_sync_and_are_deterministic():
    from isfusion_amd import nms
    head = _head("rotate")
    preds, head.query_labels = _batched_preds()
    runs = []
    for _ in range(2):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            boxes, scores, labels, counts, keep = head.decode_and_nms(preds)
            V, P, D = boxes.shape
            mapped = boxes.reshape(V * P, D).clone()
            nms.mapping_back_(mapped, V, P, [1.0, 1.0], [False, True], [True, False])
            lab = torch.where(keep, labels, torch.full_like(labels, -1)).view(-1)
            seg = nms.segmented_nms(mapped, scores.reshape(-1), ["rotate"] * 10, [0.2] * 10, V * P, labels=lab,
                                    task_of_class=list(range(10)))
        finally:
            torch.cuda.set_sync_debug_mode(0)
        runs.append((keep.clone(), seg[0].clone(), seg[1].clone(), seg[2].clone()))
    k = runs[0][3].cpu()
    for c in range(10):
        n = int(k[c])
        assert torch.equal(runs[0][2][c, :n], runs[1][2][c, :n])
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][3], runs[1][3])


def test_aug_test_is_bit_identical_run_to_run():
    net, pts, metas, img, args = _views(2)
    a = net.aug_test(pts, metas, img, **args)[0]["pts_bbox"]
    b = net.aug_test(pts, metas, img, **args)[0]["pts_bbox"]
    for k in a:
        assert torch.equal(a[k], b[k]), k
