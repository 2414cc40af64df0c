"""GPU tests of the GT-paste: isf_assemble_points_paste through MultiSweepPointLoader(paste=...) and isf_image_paste
through MultiViewImageLoader(paste=...), against what the reference's ObjectSampleV2 / MMDataBaseSamplerV2 give
(tests/golden/gt_paste_ref.npz), bit for bit.  The plans come from replaying the recorded calls on the host
(tests/test_gt_paste.py pins that replay).  Goldens only: no reference tree."""
import os

import numpy as np
import pytest
import torch

import gt_paste_common as gc
from isfusion_amd import _lib, gt_paste
from isfusion_amd import input_pipeline as ip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FINAL_DIM = (48, 128)


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "gt_paste_ref.npz"))


@pytest.fixture(scope="module")
def runs(ref):
    return gc.replay(ref)


def _points(device=DEV, ranged=False):
    return ip.MultiSweepPointLoader(sweeps_num=10, test_mode=True, device=device,
                                    point_cloud_range=gc.PC_RANGE if ranged else None)


def _images():
    return ip.MultiViewImageLoader(final_dim=FINAL_DIM, resize_lim=[0.8, 1.0], bot_pct_lim=[0.0, 0.0],
                                   rot_lim=[-5.4, 5.4], rand_flip=True, is_train=True, mean=[0.485, 0.456, 0.406],
                                   std=[0.229, 0.224, 0.225], device=DEV)


def _draws(loader, samples):
    np.random.seed(41)
    return [[loader.sample_augmentation((gc.IMG_W, gc.IMG_H)) for _ in range(gc.NUM_VIEWS)] for _ in range(samples)]


# points -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["f0", "f1", "sw", "l0"])
def test_pasted_points_equal_the_reference(ref, runs, case):
    """objects first, in plan order, then the frame without the points inside a sampled box; `sw` has two previous
    sweeps, whose points are tested after the sensor pose"""
    run = runs[case]
    got = _points()([gc.as_results(run["frame"])], paste=[run["plan"]])[0].cpu().numpy()
    want = ref[f"{case}.points"]
    assert got.shape == want.shape, f"kept {got.shape[0]} points, the reference {want.shape[0]}"
    assert np.array_equal(got, want)
    n_obj = sum(np.asarray(o["points"]).size // 5 for o in run["plan"].objects)
    assert np.any(got[:n_obj, 4] != 0) and not np.any(got[n_obj:n_obj + 100, 4] != 0)   # fifth column kept / key frame 0


@pytest.mark.parametrize("case", ["f0", "sw"])
def test_pasted_points_through_augmentation_and_range_filter(ref, runs, case):
    """both kinds of points go through the augmentation and the range filter after the paste.  The draw is a quarter
    turn with dyadic translation and scale, so the reference's float32 matmul is exact in any summation order."""
    run = runs[case]
    got = _points(ranged=True)([gc.as_results(run["frame"])], aug=[gc.AUG], paste=[run["plan"]])[0].cpu().numpy()
    want = ref[f"{case}.points_aug"]
    assert got.shape == want.shape and np.array_equal(got, want)


def test_mixed_batch_and_batch_composition(ref, runs):
    """a plan, no plan and the all-collide frame in one call; the batch call equals the per-sample calls"""
    loader = _points(ranged=True)
    cases = ["f0", "f1", "f2", "sw"]
    frames = [gc.as_results(runs[c]["frame"]) for c in cases]
    plans = [runs["f0"]["plan"], None, runs["f2"]["plan"], runs["sw"]["plan"]]
    assert plans[2] is None
    aug = [gc.AUG, None, gc.AUG, gc.AUG]
    batch = [p.cpu().numpy() for p in loader(frames, aug=aug, paste=plans)]
    assert np.array_equal(batch[0], ref["f0.points_aug"]) and np.array_equal(batch[3], ref["sw.points_aug"])
    plain = [p.cpu().numpy() for p in loader(frames, aug=aug)]
    assert np.array_equal(batch[1], plain[1]) and np.array_equal(batch[2], plain[2])
    assert batch[0].shape != plain[0].shape
    for b in range(len(cases)):
        single = loader([frames[b]], aug=[aug[b]], paste=[plans[b]])[0].cpu().numpy()
        assert np.array_equal(single, batch[b]), cases[b]
    again = [p.cpu().numpy() for p in loader(frames, aug=aug, paste=plans)]
    assert all(np.array_equal(a, b) for a, b in zip(again, batch))


@pytest.mark.parametrize("ranged", [False, True])
def test_no_plans_is_the_old_entry_bit_for_bit(runs, ranged):
    loader = _points(ranged=ranged)
    frames = [gc.as_results(runs[c]["frame"]) for c in ("f0", "sw", "l0")]
    aug = [gc.AUG, None, gc.AUG] if ranged else None
    old = loader(frames, aug=aug)
    new = loader(frames, aug=aug, paste=[None] * 3)
    assert all(torch.equal(a, b) for a, b in zip(old, new))


def test_more_than_64_boxes_is_an_error_not_a_launch(runs):
    run = runs["f0"]
    planes = np.tile(run["plan"].planes[:1], (_lib.PASTE_MAX_BOXES + 1, 1, 1))
    plan = gt_paste.GTPastePlan(objects=[], planes=planes, image_ops=[], mixup=0.7)
    with pytest.raises(_lib.IsfError, match="65 removal boxes"):
        _points()([gc.as_results(run["frame"])], paste=[plan])
    plan.planes = planes[:_lib.PASTE_MAX_BOXES]                  # 64 fit
    out = _points()([gc.as_results(run["frame"])], paste=[plan])[0]
    assert 0 < out.shape[0] < run["frame"]["points"].shape[0]


# images -------------------------------------------------------------------------------------------------------------
IMG_CASES = ["f0", "f1", "sw"]


def _image_batch(runs, cases):
    return [dict(img=runs[c]["frame"]["img"]) for c in cases], [runs[c]["plan"] for c in cases]


def test_staged_images_equal_the_reference_after_the_paste(ref, runs):
    """isf_image_paste in place on the uploaded bytes: every view of every sample equals what the reference's far-to-near
    loop leaves (real-GT mix-back, clipped patches, overlapping rectangles, skipped cameras); a sample without a plan
    and the bytes of the patches behind the images stay as uploaded"""
    loader = _images()
    cases = IMG_CASES + ["f2"]
    results, plans = _image_batch(runs, cases)
    staged = loader.stage(results, aug=_draws(loader, len(cases)), paste=plans)
    before = staged["raw"].cpu().numpy().copy()
    loader.paste(staged)
    after = staged["raw"].cpu().numpy()
    per = gc.NUM_VIEWS * gc.IMG_H * gc.IMG_W * 3
    for b, c in enumerate(cases):
        got = after[b * per:(b + 1) * per].reshape(gc.NUM_VIEWS, gc.IMG_H, gc.IMG_W, 3)
        want = ref[f"{c}.img"] if c != "f2" else np.stack(runs[c]["frame"]["img"])
        bad = int((got != want).sum())
        assert bad == 0, f"{c}: {bad} bytes differ from the reference"
        if c != "f2":
            assert (got != np.stack(runs[c]["frame"]["img"])).any()
    assert after.size > len(cases) * per and np.array_equal(after[len(cases) * per:], before[len(cases) * per:])


def test_loader_with_plans_equals_loader_on_pasted_images(ref, runs):
    loader = _images()
    results, plans = _image_batch(runs, IMG_CASES)
    draws = _draws(loader, len(IMG_CASES))
    got, mats = loader(results, aug=draws, paste=plans)
    pasted = [dict(img=list(ref[f"{c}.img"])) for c in IMG_CASES]
    want, want_mats = loader(pasted, aug=draws)
    assert torch.equal(got, want) and torch.equal(mats, want_mats)
    plain, _ = loader(results, aug=draws)
    assert not torch.equal(got, plain)
    for b in range(len(IMG_CASES)):                              # batch composition
        single, _ = loader([results[b]], aug=[draws[b]], paste=[plans[b]])
        assert torch.equal(single[0], got[b])


def test_image_paste_makes_no_host_sync_and_is_deterministic(runs):
    loader = _images()
    results, plans = _image_batch(runs, IMG_CASES)
    draws = _draws(loader, len(IMG_CASES))
    first, _ = loader(results, aug=draws, paste=plans)          # pins the staging buffers
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second, _ = loader(results, aug=draws, paste=plans)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(first, second)


def test_lidar_only_plan_touches_no_image(runs):
    loader = _images()
    results = [dict(img=runs["l0"]["frame"]["img"])]
    draws = _draws(loader, 1)
    staged = loader.stage(results, aug=draws, paste=[runs["l0"]["plan"]])
    assert "paste" not in staged
    a, _ = loader(results, aug=draws, paste=[runs["l0"]["plan"]])
    b, _ = loader(results, aug=draws)
    assert torch.equal(a, b)


def test_more_than_256_operations_is_an_error_not_a_launch(runs):
    loader = _images()
    op = dict(view=0, kind="mix", rows=(0, 4), cols=(0, 4))
    plan = gt_paste.GTPastePlan(objects=[], planes=np.zeros((0, 6, 4), np.float32), mixup=0.7,
                                image_ops=[dict(op) for _ in range(_lib.PASTE_MAX_OPS + 1)])
    results = [dict(img=runs["f0"]["frame"]["img"])]
    with pytest.raises(_lib.IsfError, match="257 operations"):
        loader.stage(results, aug=_draws(loader, 1), paste=[plan])
    rc = _lib.load().isf_image_paste(None, None, 6, None, _lib.PASTE_MAX_OPS + 1, 4, 4, 0.7, 0.3, 0.7, None)
    assert rc == -4
    plan.image_ops = plan.image_ops[:_lib.PASTE_MAX_OPS]        # 256 are walked: 0.7 v + 0.3 v, 256 times, is v or v - 1
    staged = loader.stage(results, aug=_draws(loader, 1), paste=[plan])
    loader.paste(staged)
    got = staged["raw"][:gc.IMG_H * gc.IMG_W * 3].cpu().numpy().reshape(gc.IMG_H, gc.IMG_W, 3)
    want = runs["f0"]["frame"]["img"][0].copy()
    v = want[:4, :4].astype(np.float64)
    o = v.copy()
    for _ in range(_lib.PASTE_MAX_OPS):
        v = (0.7 * o + (1 - 0.7) * v).astype(np.uint8).astype(np.float64)
    want[:4, :4] = v.astype(np.uint8)
    assert np.array_equal(got, want)


# downstream ---------------------------------------------------------------------------------------------------------
def test_pasted_sample_feeds_the_voxelizer(runs):
    """plumbing only: the pasted points and the concatenated boxes of one plan go through a drawn training
    augmentation, augment_gt_boxes and the voxelizer"""
    import isfusion_amd as m
    run = runs["f0"]
    np.random.seed(9)
    aug = ip.draw_train_aug()
    rng = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
    loader = ip.MultiSweepPointLoader(test_mode=True, point_cloud_range=rng, device=DEV)
    pts = loader([gc.as_results(run["frame"])], aug=[aug], paste=[run["plan"]])[0]
    boxes, labels = ip.augment_gt_boxes(run["plan"].gt_bboxes_3d, run["plan"].gt_labels_3d, aug, rng, len(gc.CLASSES))
    assert boxes.shape[1] == 9 and 0 < boxes.shape[0] <= len(run["plan"].gt_labels_3d) and len(labels) == boxes.shape[0]
    assert len(labels) > len(run["frame"]["gt_labels_3d"]) - 2 and torch.isfinite(boxes).all()
    assert torch.isfinite(pts).all() and pts.shape[0] > 4000
    voxels, coors, num = m.voxelization(pts.contiguous(), [0.075, 0.075, 0.2], rng, 10, 60000)
    assert voxels.shape[0] > 1000 and int(num.sum()) <= pts.shape[0] and torch.isfinite(voxels).all()
