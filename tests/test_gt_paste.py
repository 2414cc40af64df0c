"""Host side of the GT-paste (isfusion_amd.gt_paste) against the reference's ObjectSampleV2 / MMDataBaseSamplerV2 /
ModalMask3D, recorded in tests/golden/gt_paste_ref.npz by tests/golden/make_golden_gt_paste.py.  No GPU."""
import ast
import os
import random
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
GOLDEN = os.path.join(HERE, "golden")

import gt_paste_common as gc  # noqa: E402
from isfusion_amd import _lib, gt_paste  # noqa: E402

CASES = [c[0] for c in gc.CALLS]


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "gt_paste_ref.npz"))


@pytest.fixture(scope="module")
def runs(ref):
    return gc.replay(ref)


def _gids(run, name, indices):
    return [run["db"][name][int(i)]["gid"] for i in indices]


# 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_sampler_draws_the_reference_objects(ref, runs, case):
    """same candidates in the same order per class call, same valid_samples, same collision matrices (the drawn
    threshold included), and the numpy RNG left where the reference leaves it"""
    run = runs[case]
    assert len(run["debug"]) == int(ref[f"{case}.calls"])
    for k, rec in enumerate(run["debug"]):
        assert gc.CLASSES.index(rec["name"]) == int(ref[f"{case}.{k}.name"])
        assert _gids(run, rec["name"], rec["indices"]) == list(ref[f"{case}.{k}.sampled"])
        assert _gids(run, rec["name"], rec["indices"][rec["valid"]]) == list(ref[f"{case}.{k}.valid"])
        off = ~np.eye(len(rec["coll_bev"]), dtype=bool)      # the reference clears the diagonal before it reads it
        assert np.array_equal(rec["coll_bev"][off], ref[f"{case}.{k}.bev"][off])
        if f"{case}.{k}.c2d" in ref:
            assert rec["collision_thr"] == float(ref[f"{case}.{k}.thr"])
            assert np.array_equal(rec["coll_2d"][off], ref[f"{case}.{k}.c2d"][off])
        else:
            assert rec["coll_2d"] is None
    assert run["next_rand"] == float(ref[f"{case}.next_rand"])
    assert (run["plan"] is None) == bool(ref[f"{case}.none"])


def test_recorded_calls_cover_both_threshold_kinds_and_every_class(ref):
    thr = [float(ref[k]) for k in ref.files if k.endswith(".thr")]
    assert 0.0 in thr and any(t > 0 for t in thr)
    assert {int(ref[k]) for k in ref.files if k.endswith(".name")} == set(range(10))


def test_a_box_wholly_inside_another_collides(ref, runs):
    """numba's `is` compares values: the containment branch of box_collision_test runs.  Frame 0's bus holds database
    cone 0 with no edge crossing; the pair is in the recorded matrix and in ours."""
    rec = next(r for r in runs["f0"]["debug"] if r["name"] == "traffic_cone")
    k = runs["f0"]["debug"].index(rec)
    cone = [runs["f0"]["db"]["traffic_cone"][int(i)]["gid"] for i in rec["indices"]].index(
        runs["f0"]["db"]["traffic_cone"][0]["gid"])
    G = len(runs["f0"]["frame"]["gt_bboxes_3d"])
    assert rec["coll_bev"][G + cone, 0] and rec["coll_bev"][0, G + cone]      # the bus is ground-truth box 0
    assert ref[f"f0.{k}.bev"][G + cone, 0]
    assert not rec["valid"][cone]
    # the pair really has no crossing edges: moving the cone to the bus's centre keeps it a collision
    big = np.array([[[-6, -2], [-6, 2], [6, 2], [6, -2]]], np.float64)
    small = big / 20
    assert gt_paste.box_collision_test(big, small)[0, 0] and gt_paste.box_collision_test(small, big)[0, 0]
    assert not gt_paste.box_collision_test(big, small + 30)[0, 0]


def test_frame_with_too_many_cars_samples_no_car(runs):
    assert "car" not in [r["name"] for r in runs["f1"]["debug"]]
    assert "car" in [r["name"] for r in runs["f0"]["debug"]]


def test_batch_sampler_wraps_round(runs):
    """a class with no more entries than its sample_groups number hands out its whole list and reshuffles, every call"""
    recs = [[r for r in runs[c]["debug"] if r["name"] == "construction_vehicle"][0] for c in ("f0", "f1", "sw")]
    for r in recs:
        assert sorted(r["indices"]) == list(range(gc.DB_COUNTS["construction_vehicle"]))
    assert len({tuple(r["indices"]) for r in recs}) > 1
    np.random.seed(3)
    bs = gt_paste.BatchSampler(list("abcde"), "x")
    first = bs._sample(2).copy()                            # a view of the indices the reshuffle below permutes
    assert len(first) == 2 and bs._idx == 2
    tail = bs._sample(3)                                    # _idx + num >= len: the tail, then a reshuffle
    assert len(tail) == 3 and bs._idx == 0 and sorted(list(first) + list(tail)) == [0, 1, 2, 3, 4]


def test_filters_drop_the_marked_entries(runs):
    for name, infos in runs["f0"]["db"].items():
        assert len(infos) == gc.DB_COUNTS[name]
        assert all(i["difficulty"] != -1 and i["num_points_in_gt"] >= 5 for i in infos)


# 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_ground_truth_after_the_call(ref, runs, case):
    res, plan = runs[case]["result"], runs[case]["plan"]
    got = res["gt_bboxes_3d"]
    assert got.dtype == np.float32 and np.array_equal(got, ref[f"{case}.gt_bboxes_3d"])
    assert np.array_equal(res["gt_labels_3d"], ref[f"{case}.gt_labels_3d"])
    if case == "stop":                                      # the reference returns before it touches anything
        assert res["gt_bboxes"].shape[1] == 5 and "gt_labels" not in res
    elif "gt_bboxes" in res:
        assert res["gt_bboxes"].shape[1] == 4               # cut to [:, :4] even when nothing was valid
        assert np.array_equal(res["gt_bboxes"], ref[f"{case}.gt_bboxes"])
        assert np.array_equal(res["gt_labels"], ref[f"{case}.gt_labels"])
    if plan is not None:
        assert np.array_equal(plan.gt_bboxes_3d, ref[f"{case}.gt_bboxes_3d"])
        assert np.array_equal(plan.gt_labels_3d, ref[f"{case}.gt_labels_3d"])
        assert len(plan.objects) == len(plan.planes) == len(plan.gt_labels_3d) - len(runs[case]["frame"]["gt_labels_3d"])
        for obj, box in zip(plan.objects, plan.sampled_gt_bboxes_3d):
            assert obj["translation"].dtype == np.float32 and np.array_equal(obj["translation"], box[:3])


def test_stop_epoch_and_all_collide_return_none(runs):
    assert runs["stop"]["plan"] is None and runs["stop"]["debug"] == []
    assert runs["f2"]["plan"] is None and len(runs["f2"]["debug"]) == 10
    assert not any(r["valid"].any() for r in runs["f2"]["debug"])


def test_lidar_only_sampler_touches_no_image(runs):
    plan = runs["l0"]["plan"]
    assert plan.image_ops == [] and plan.gt_bboxes is None and all(o["patch"] is None for o in plan.objects)
    assert plan.gt_bboxes_3d.shape[1] == 7


@pytest.mark.parametrize("case", ["f0", "f1", "sw", "l0"])
def test_plane_equations(ref, runs, case):
    want = ref[f"{case}.planes"]
    got = runs[case]["plan"].planes
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.abs(got - want).max() <= 1e-6


def test_planes_classify_points():
    box = np.array([[1.0, 2.0, -1.0, 4.0, 2.0, 1.5, 0.4]], np.float32)         # z is the bottom face: origin (.5, .5, 0)
    planes = gt_paste.box_planes(box)[0].astype(np.float64)
    along = np.array([np.cos(0.4), -np.sin(0.4), 0.0])                        # the box's length axis (clockwise yaw)
    inside = [np.array([1.0, 2.0, -0.5]), np.array([1.0, 2.0, -0.5]) + 1.9 * along]
    outside = [np.array([1.0, 2.0, -1.1]), np.array([1.0, 2.0, 0.6]), np.array([1.0, 2.0, -0.5]) + 2.1 * along]
    for p in inside:
        assert (planes[:, :3] @ p + planes[:, 3] < 0).all()
    for p in outside:
        assert not (planes[:, :3] @ p + planes[:, 3] < 0).all()


# 3 ------------------------------------------------------------------------------------------------------------------
def test_image_operations(runs):
    """far-to-near order with the reference's inverse-permutation quirk, rows = x1:x2 for real ground truth, skipped
    cameras, clipped patches"""
    run = runs["f0"]
    plan, fr = run["plan"], run["frame"]
    all_3d = plan.gt_bboxes_3d
    cam = np.concatenate([fr["gt_bboxes"][:, 4], [run["db"][o["name"]][o["index"]]["box2d_camera"][4]
                                                  for o in plan.objects]])
    order = np.argsort(-all_3d[:, 0])
    expected = [int(np.where(order == idx)[0][0]) for idx in range(len(all_3d))]
    expected = [i for i in expected if cam[i] < gc.SAMPLER_KW["img_num"]]
    G = len(fr["gt_bboxes"])
    got = []
    for op in plan.image_ops:
        assert 0 <= op["rows"][0] < op["rows"][1] <= gc.IMG_H and 0 <= op["cols"][0] < op["cols"][1] <= gc.IMG_W
        got.append(op)
    kinds = [("mix" if i < G else "patch") for i in expected]
    # real-GT rectangles that clip to nothing leave no operation
    assert [op["kind"] for op in got if op["kind"] == "patch"] == [k for k in kinds if k == "patch"]
    assert [G + op["object"] for op in got if op["kind"] == "patch"] == [i for i in expected if i >= G]
    assert all(op["view"] < gc.SAMPLER_KW["img_num"] for op in got)
    assert any(cam[i] >= gc.SAMPLER_KW["img_num"] for i in range(G, len(all_3d))), "no object on a skipped camera"
    for op in got:
        if op["kind"] == "mix":
            i = [j for j in range(G) if int(fr["gt_bboxes"][j, 4]) == op["view"]
                 and gt_paste.resolve_slice(int(fr["gt_bboxes"][j, 0]), int(fr["gt_bboxes"][j, 2]), gc.IMG_H) == op["rows"]]
            assert i, "a real-GT operation indexes rows by x1:x2"
    every = [op for c in ("f0", "f1", "sw") for op in runs[c]["plan"].image_ops]
    assert any(op["kind"] == "patch" and op["rows"][1] == gc.IMG_H and op["cols"][1] == gc.IMG_W for op in every)
    frames = [runs[c]["frame"]["gt_bboxes"] for c in ("f0", "f1", "sw")]
    assert any(int(b[2]) > gc.IMG_H for f in frames for b in f), "no real-GT rectangle with x2 > H"


def test_rectangles_resolve_like_numpy_slices():
    rng = np.random.default_rng(0)
    for _ in range(2000):
        size = int(rng.integers(1, 40))
        a, b = (int(v) for v in rng.integers(-3 * size, 3 * size, 2))
        begin, end = gt_paste.resolve_slice(a, b, size)
        want = np.arange(size)[a:b]
        assert end - begin == len(want) and (len(want) == 0 or (begin == want[0] and end == want[-1] + 1))
        assert 0 <= begin <= end <= size


# 4 ------------------------------------------------------------------------------------------------------------------
def test_from_config_reads_the_shipped_pipeline(ref, tmp_path):
    with open(os.path.join(GOLDEN, "isfusion_0075voxel_pipelines.txt")) as f:
        text = f.read()
    cfg = ast.literal_eval(text)
    db = gc.database(int(ref["seed"]))
    path = tmp_path / "cfg.py"
    path.write_text("both = " + text + "train_pipeline = both['train_pipeline']\ntest_pipeline = both['test_pipeline']\n")
    for config in (cfg, (cfg["train_pipeline"], cfg["test_pipeline"]), str(path)):
        np.random.seed(0)
        s = gt_paste.GTPasteSampler.from_config(config, db_infos=db)
        assert s.sample_2d and s.stop_epoch == 8 and s.epoch == -1
        assert s.mixup == 0.7 and s.img_num == 6 and s.rate == 1.0 and s.check_2D_collision and s.depth_consistent
        assert s.collision_thr == [0, 0.3, 0.5, 0.7] and not s.collision_in_classes and s.blending_type is None
        assert s.classes == gc.CLASSES and s.data_root == "data/nuscenes/"
        assert s.info_path == "data/nuscenes/nuscenes_dbinfos_train.pkl"
        assert dict(zip(s.sample_classes, s.sample_max_nums)) == gc.SAMPLE_GROUPS
        assert s.sample_classes[:3] == ["car", "truck", "construction_vehicle"]       # the config's order, not sorted
        assert s.prepare == gc.PREPARE
    s.set_epoch(8)
    assert s.sample(gc.sample_input(gc.frame(int(ref["seed"]), 0, db))) is None


def test_raising_cases(ref):
    db = gc.database(int(ref["seed"]))
    with pytest.raises(_lib.IsfError, match="blending_type"):
        gt_paste.GTPasteSampler(db_infos=db, **dict(gc.SAMPLER_KW, blending_type=["box"]))
    with pytest.raises(_lib.IsfError):
        gt_paste.GTPasteSampler(**gc.SAMPLER_KW)                                     # neither db_infos nor info_path
    with pytest.raises(_lib.IsfError):
        gt_paste.GTPasteSampler(db_infos=db, **dict(gc.SAMPLER_KW, points_loader=dict(load_dim=4, use_dim=[0, 1, 2, 3])))
    # a patch that does not cover its (unclipped) box: numpy cannot broadcast it -> raised before any launch
    fr = gc.frame(int(ref["seed"]), 0, db)
    for infos in db.values():
        for i in infos:
            i["patch"] = i["patch"][:2, :2]
    np.random.seed(1)
    s = gt_paste.GTPasteSampler(db_infos=db, sample_2d=True, **gc.SAMPLER_KW)
    with pytest.raises(_lib.IsfError, match="patch"):
        for _ in range(4):
            s.sample(gc.sample_input(fr))
    # a box whose left edge is off the image wraps to an empty region
    bad = gc.database(int(ref["seed"]))
    for infos in bad.values():
        for i in infos:
            i["box2d_camera"][[0, 2]] -= 200
    np.random.seed(1)
    s = gt_paste.GTPasteSampler(db_infos=bad, sample_2d=True, **dict(gc.SAMPLER_KW, check_2D_collision=False))
    with pytest.raises(_lib.IsfError):
        s.sample(gc.sample_input(fr))


def test_database_from_files(ref, tmp_path):
    """info_path pickle, point files under data_root and path + '.png' patches give the plan the arrays give"""
    import pickle
    from PIL import Image
    seed = int(ref["seed"])
    db, disk = gc.database(seed), {}
    for name, infos in db.items():
        disk[name] = []
        for i in infos:
            rel = f"obj_{i['gid']}.bin"
            i["path"].tofile(str(tmp_path / rel))
            Image.fromarray(i["patch"]).save(str(tmp_path / (rel + ".png")))
            disk[name].append(dict({k: v for k, v in i.items() if k != "patch"}, path=rel))
    with open(tmp_path / "infos.pkl", "wb") as f:
        pickle.dump(disk, f)
    fr = gc.frame(seed, 0, db)
    plans = []
    for kw in (dict(db_infos=db), dict(info_path=str(tmp_path / "infos.pkl"), data_root=str(tmp_path))):
        np.random.seed(5)
        s = gt_paste.GTPasteSampler(sample_2d=True, **gc.SAMPLER_KW, **kw)
        plans.append(s.sample(gc.sample_input(fr)))
    a, b = plans
    assert len(a.objects) == len(b.objects) > 0 and a.image_ops == b.image_ops
    for x, y in zip(a.objects, b.objects):
        assert isinstance(y["points"], str) and np.array_equal(np.fromfile(y["points"], np.float32), x["points"].reshape(-1))
        assert (x["patch"] is None and y["patch"] is None) or np.array_equal(x["patch"], y["patch"])


# 5 ------------------------------------------------------------------------------------------------------------------
def test_draw_modal_mask(ref):
    for k, (a, b) in enumerate(ref["modal.seeds"]):
        np.random.seed(int(a))
        random.seed(int(b))
        assert gt_paste.draw_modal_mask(gc.NUM_VIEWS, mode="train") == list(ref[f"modal.{k}"])
    assert gt_paste.draw_modal_mask(gc.NUM_VIEWS, mode="test") == list(ref["modal.test"]) == [0]
    np.random.seed(1)
    random.seed(1)
    assert len(gt_paste.draw_modal_mask(6, "train", dataset_type="KittiDataset")) == 2


# 6 ------------------------------------------------------------------------------------------------------------------
def test_new_entries_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "isf_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in ("isf_assemble_points_paste", "isf_image_paste"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    for name, value in (("ISF_SWEEP_PASTED", _lib.SWEEP_PASTED), ("ISF_PASTE_MAX_BOXES", _lib.PASTE_MAX_BOXES),
                        ("ISF_PASTE_MAX_OPS", _lib.PASTE_MAX_OPS), ("ISF_PASTE_MIX", _lib.PASTE_MIX),
                        ("ISF_PASTE_PATCH", _lib.PASTE_PATCH)):
        assert int(re.search(r"^#define " + name + r"\s+(\d+)", hdr, flags=re.M).group(1)) == value
    assert (_lib.PASTE_MAX_BOXES, _lib.PASTE_MAX_OPS) == (64, 256)
    import ctypes
    assert ctypes.sizeof(_lib.PasteView) == 40 and ctypes.sizeof(_lib.PasteOp) == 48


def test_paste_entries_refuse_what_they_cannot_hold():
    """the limit checks sit in front of every HIP call: they answer without a GPU"""
    import ctypes
    lib = _lib.load()
    offsets = (ctypes.c_int32 * 2)(0, _lib.PASTE_MAX_BOXES + 1)
    planes = (ctypes.c_float * (24 * (_lib.PASTE_MAX_BOXES + 1)))()
    sample_offsets = ctypes.c_void_p(8)      # never dereferenced: the check comes first
    rc = lib.isf_assemble_points_paste(None, None, 0, 1, None, None, planes, offsets, None, sample_offsets, None, None)
    assert rc == -4 and b"65 removal boxes" in lib.isf_last_error()
    rc = lib.isf_image_paste(None, None, 1, None, _lib.PASTE_MAX_OPS + 1, 8, 8, 0.7, 0.3, 0.7, None)
    assert rc == -4 and b"257 operations" in lib.isf_last_error()
