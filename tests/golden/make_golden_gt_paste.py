"""Generate tests/golden/gt_paste_ref.npz: the REFERENCE's multi-modal GT-paste -- transforms_3d.ObjectSampleV2 over
dbsampler.MMDataBaseSamplerV2 (and, for sample_2d=False, the plain DataBaseSampler it defaults to), with
data_augment_utils.box_collision_test and box_np_ops, and transforms_3d.ModalMask3D -- on the seeded inputs of
tests/gt_paste_common.py.

    python tests/golden/make_golden_gt_paste.py            # authoring container only

The reference's own files are loaded through ref_harness.install_pipelines() plus stubs for what is absent here:
numba and numba.errors (jit / njit are identity decorators: the functions run as plain Python), mmdet3d.utils, and
mmcv.load / mmcv.build_from_cfg.  Stand-ins: LoadImageFromFile (Pillow -> a BGR array, as mmcv returns), and the
gt_bboxes_3d holder (`.tensor`, `.new_box`; LiDARInstance3DBoxes needs the compiled box ops).  The points loader is the
reference's own LoadPointsFromFile, and every frame first goes through its LoadPointsFromMultiSweeps.

numba's `is` semantics: compiled, `ret[i, j] is True` in box_collision_test compares VALUES, so the full-containment
branch runs; as plain Python on numpy bools it never fires.  To get the compiled behaviour out of the reference's own
text, data_augment_utils' module-level `np` is a thin proxy whose zeros(..., dtype=np.bool_) returns an object array
of Python bools (`is True` then holds exactly when the value is True); everything else passes through.  Every BEV
matrix is cross-checked against an independent float64 separating-axes overlap test written here, and the golden is
required to hold a pair that collides by containment alone (without the proxy it comes out False).  The 2D matrices at
collision_thr == 0 come from corners in the order (x1y1, x2y1, x1y2, x2y2), which is no polygon order: they are the
reference's, not a geometric overlap, and are only required to be a subset of the true overlaps; their count of
misses is printed.

Conditions on the inputs (asserted; the seed is re-drawn until they hold) make every comparison exact without
depending on the last bit of a numpy build: no scene point within 1e-3 m of a face of a sampled box (float64), no
decision of a collision test changing when every box grows or shrinks by 1e-3 (m in BEV, pixels in 2D), no iof within
1e-4 of the drawn threshold.

Stored, per recorded call `c` of gt_paste_common.CALLS (shapes: G ground-truth boxes, S valid samples, T = G + the
class call's candidates):
  c.calls                       number of sample_class calls
  c.k.name / .sampled / .valid  class label, gids of the candidates [n], gids of the valid ones [<= n]
  c.k.bev / .c2d / .thr         collision matrices bool [T, T] (c2d absent without the 2D test), the drawn threshold
  c.points                      float32 [N, 5]   result points (pasted objects first)
  c.points_aug                  float32 [M, 5]   the same through the crafted augmentation (gt_paste_common.AUG: the
                                reference's LiDARPoints.rotate / translate / scale / flip) and PointsRangeFilter
  c.gt_bboxes_3d / .gt_labels_3d / .gt_bboxes / .gt_labels      the result dict's ground truth
  c.img                         uint8 [6, 96, 160, 3]   every view (RGB), only for calls that pasted
  c.planes                      float32 [S, 6, 4]   plane equations of the sampled boxes (surface_equ_3d)
  c.none                        1 when the call left the points alone (stop_epoch, nothing valid)
  c.next_rand                   np.random.rand() right after the call
  seed                          the inputs' seed;  modal.*  the ModalMask3D draws"""
import os
import pickle
import random
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gt_paste_common as gc  # noqa: E402
import ref_harness  # noqa: E402

FIRST_SEED = 2024
MODAL_SEEDS = [(3, 5), (4, 6), (9, 1), (12, 2)]


class _NpProxy:
    """numpy for data_augment_utils: zeros(dtype=np.bool_) -> an object array of Python bools (see the docstring)"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def zeros(shape, dtype=float, **kw):
        if dtype is np.bool_:
            out = np.empty(shape, dtype=object)
            out.fill(False)
            return out
        return np.zeros(shape, dtype=dtype, **kw)


class _Boxes:
    """gt_bboxes_3d holder: what ObjectSampleV2 reads of LiDARInstance3DBoxes"""

    def __init__(self, data):
        self.tensor = torch.as_tensor(np.asarray(data), dtype=torch.float32)

    def new_box(self, data):
        return _Boxes(data)


class _LoadImageFromFile:
    """mmdet's LoadImageFromFile for a patch file: BGR uint8, as mmcv.imread returns"""

    def __init__(self, **kw):
        pass

    def __call__(self, results):
        with Image.open(results["img_info"]["filename"]) as im:
            results["img"] = np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])
        return results


def install():
    ref = ref_harness.install_pipelines()
    ident = ref_harness._identity_decorator

    def jit(*a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]
        return ident(*a, **k)

    ref_harness._mod("numba", jit=jit, njit=jit)
    ref_harness._mod("numba.errors", NumbaPerformanceWarning=UserWarning)
    ref_harness._mod("mmdet3d.utils", get_root_logger=lambda *a, **k: types.SimpleNamespace(info=lambda *a, **k: None))
    mmcv = sys.modules["mmcv"]
    mmcv.build_from_cfg = lambda cfg, reg: reg.build(cfg)

    def load(path):
        with open(path, "rb") as f:
            return pickle.load(f)
    mmcv.load = load
    pipelines = sys.modules["mmdet.datasets.builder"].PIPELINES
    pipelines.module_dict["LoadImageFromFile"] = _LoadImageFromFile
    sys.modules["mmdet.datasets"].PIPELINES = pipelines
    ops = ref_harness._load("mmdet3d.core.bbox.box_np_ops", "mmdet3d/core/bbox/box_np_ops.py")
    bbox = sys.modules["mmdet3d.core.bbox"]
    bbox.box_np_ops, bbox.LiDARInstance3DBoxes = ops, _Boxes
    dau = ref_harness._load("mmdet3d.datasets.pipelines.data_augment_utils",
                            "mmdet3d/datasets/pipelines/data_augment_utils.py")
    sys.modules["mmdet3d.datasets.pipelines"].data_augment_utils = dau
    dbs = ref_harness._load("mmdet3d.datasets.pipelines.dbsampler", "mmdet3d/datasets/pipelines/dbsampler.py")
    T = ref["transforms_3d"]
    T.box_np_ops = ops
    T.build_from_cfg = lambda cfg, reg: reg.build(cfg)
    return dict(ref, box_np_ops=ops, data_augment_utils=dau, dbsampler=dbs)


# ---------------------------------------------------------------------------------------------- independent checks
def sat_overlap(a, b):
    """float64 separating-axes test of two convex quadrilaterals [4, 2] (corners in polygon order): positive-area
    overlap, containment included"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    for poly in (a, b):
        for k in range(4):
            edge = poly[(k + 1) % 4] - poly[k]
            axis = np.array([-edge[1], edge[0]])
            pa, pb = a @ axis, b @ axis
            if pa.max() <= pb.min() or pb.max() <= pa.min():
                return False
    return True


def bev_corners(boxes, grow=0.0):
    """float64 BEV corners of [x, y, z, dx, dy, dz, yaw] boxes in polygon order, each side moved out by `grow`"""
    out = []
    for b in np.asarray(boxes, np.float64):
        hx, hy = b[3] / 2 + grow, b[4] / 2 + grow
        local = np.array([[-hx, -hy], [-hx, hy], [hx, hy], [hx, -hy]])
        c, s = np.cos(b[6]), np.sin(b[6])
        out.append(local @ np.array([[c, -s], [s, c]]) + b[:2])
    return np.stack(out)


def check_call(rec, by_gid, gtp):
    """the conditions on one sample_class call + the cross-checks (off the diagonal, which the reference clears);
    -> number of true 2D overlaps the reference's corner order misses"""
    gt3d, gt2d = rec["gt3d"], rec["gt2d"]
    width = gt3d.shape[1]
    boxes3d = np.concatenate([gt3d, np.stack([by_gid[g]["box3d_lidar"][:width] for g in rec["sampled"]])])
    n = len(boxes3d)
    off = ~np.eye(n, dtype=bool)
    misses = 0
    for grow in (0.0, 1e-3, -1e-3):
        corners = bev_corners(boxes3d, grow)
        sat = np.array([[sat_overlap(corners[i], corners[j]) for j in range(n)] for i in range(n)])
        assert np.array_equal(sat[off], rec["bev"][off]), f"BEV matrix differs from the separating-axes test ({grow})"
        assert np.array_equal(gtp.box_collision_test(corners, corners)[off], rec["bev"][off])
    if rec["c2d"] is not None:
        boxes2d = np.concatenate([gt2d, np.stack([by_gid[g]["box2d_camera"] for g in rec["sampled"]])]) \
            if len(gt2d) else np.stack([by_gid[g]["box2d_camera"] for g in rec["sampled"]])
        b = boxes2d.astype(np.float64)
        for grow in (0.0, 1e-3, -1e-3):
            g = b + np.array([-grow, -grow, grow, grow, 0])
            if rec["thr"] == 0:
                corners = np.stack([g[:, [0, 1]], g[:, [2, 1]], g[:, [0, 3]], g[:, [2, 3]]], axis=1)
                assert np.array_equal(gtp.box_collision_test(corners, corners)[off], rec["c2d"][off]), \
                    "a 2D decision changes within 1e-3 px"
            else:
                assert np.array_equal((gtp.iof(g, g) > rec["thr"])[off], rec["c2d"][off]), \
                    "an iof decision changes within 1e-3 px"
        true = (np.minimum(b[:, None, 2], b[None, :, 2]) > np.maximum(b[:, None, 0], b[None, :, 0])) & \
               (np.minimum(b[:, None, 3], b[None, :, 3]) > np.maximum(b[:, None, 1], b[None, :, 1]))
        if rec["thr"] == 0:
            assert not (rec["c2d"] & ~true & off).any()
            misses = int((true & ~rec["c2d"] & off).sum())
        else:
            val = gtp.iof(b, b)
            assert (np.abs(val - rec["thr"]) > 1e-4).all(), "an iof within 1e-4 of the threshold"
    return misses


def run(seed, ref, tmp):
    import isfusion_amd.gt_paste as gtp
    L, T, dbs, dau, ops = ref["loading"], ref["transforms_3d"], ref["dbsampler"], ref["data_augment_utils"], ref["box_np_ops"]
    db = gc.database(seed)
    by_gid = {i["gid"]: i for infos in db.values() for i in infos}

    def to_disk(db, tag):
        """the database as the reference reads it: a pickle of infos whose `path` is a file, patches as PNG"""
        out = {}
        for name, infos in db.items():
            out[name] = []
            for i in infos:
                path = os.path.join(tmp, f"{tag}_{i['gid']}.bin")
                i["path"].tofile(path)
                Image.fromarray(i["patch"]).save(path + ".png")
                out[name].append(dict({k: v for k, v in i.items() if k != "patch"}, path=path))
        info_path = os.path.join(tmp, f"{tag}_infos.pkl")
        with open(info_path, "wb") as f:
            pickle.dump(out, f)
        return info_path

    store = {"seed": np.int64(seed)}
    np.random.seed(seed)
    kw = dict(gc.SAMPLER_KW, info_path=to_disk(db, "main"), data_root=None)
    main = T.ObjectSampleV2(db_sampler=dict(kw, type="MMDataBaseSamplerV2"), sample_2d=True, stop_epoch=gc.STOP_EPOCH)
    lidar_kw = {k: kw[k] for k in ("rate", "prepare", "sample_groups", "classes", "points_loader")}
    lidar = T.ObjectSampleV2(db_sampler=dict(lidar_kw, info_path=to_disk(gc.lidar_database(db), "lidar"),
                                             data_root=None), sample_2d=False)
    transforms = dict(main=main, lidar=lidar)

    # recording hooks around the reference's own functions
    log = []
    plain_collision = ref.setdefault("_collision", dau.box_collision_test)

    def collision(boxes, qboxes, clockwise=True):
        out = plain_collision(boxes, qboxes, clockwise)
        dau.np = np                                         # the same call as plain Python on numpy bools
        try:
            without = plain_collision(boxes, qboxes, clockwise)
        finally:
            dau.np = real_np
        log.append(("coll", np.asarray(out).astype(bool), np.asarray(without).astype(bool)))
        return out

    plain_iou = ref.setdefault("_iou", ops.iou_jit)

    def iou(boxes, query, mode="iou", eps=0.0):
        out = plain_iou(boxes, query, mode, eps)
        log.append(("iof", out.copy()))
        return out

    dau.np = real_np = _NpProxy()
    dau.box_collision_test, ops.iou_jit = collision, iou
    resets = []
    plain_reset = ref.setdefault("_reset", dbs.BatchSampler._reset)

    def counted_reset(self):
        resets.append(self._name)
        return plain_reset(self)
    dbs.BatchSampler._reset = counted_reset
    for t in transforms.values():
        s = t.db_sampler
        plain = s.sample_class_v2

        def sample_class(name, num, *a, _plain=plain, _s=s):
            drawn, thr = [], []
            orig, choice = _s.sampler_dict[name].sample, np.random.choice

            def sample(n):
                got = orig(n)
                drawn.extend(i["gid"] for i in got)
                return got

            def record_choice(*args, **kw):                 # the only np.random.choice of the call: collision_thr
                thr.append(choice(*args, **kw))
                return thr[-1]
            _s.sampler_dict[name].sample, np.random.choice = sample, record_choice
            start = len(log)
            try:
                valid = _plain(name, num, *a)
            finally:
                _s.sampler_dict[name].sample, np.random.choice = orig, choice
            mats = log[start:]
            rec = dict(name=name, sampled=np.array(drawn), valid=np.array([v["gid"] for v in valid], np.int64),
                       bev=mats[0][1], bev_plain=mats[0][2], c2d=None, thr=None, gt3d=np.asarray(a[0]),
                       gt2d=np.asarray(a[1]) if len(a) > 1 else None)
            if len(mats) > 1:
                assert len(thr) == 1 and (thr[0] == 0) == (mats[1][0] == "coll")
                rec.update(thr=float(thr[0]), c2d=mats[1][1] if thr[0] == 0 else mats[1][1] > thr[0],
                           iof=None if thr[0] == 0 else mats[1][1])
            calls.append(rec)
            return valid
        s.sample_class_v2 = sample_class

    thr_kinds, contain_pairs, total_misses = set(), 0, 0
    for case, which, index, epoch, rng_seed in gc.CALLS:
        fr = gc.frame(seed, index, db)
        key_path = os.path.join(tmp, f"{case}_key.bin")
        fr["points"].tofile(key_path)
        infos = []
        for k, sw in enumerate(fr["sweeps"]):
            p = os.path.join(tmp, f"{case}_sweep{k}.bin")
            sw["points"].tofile(p)
            infos.append(dict(data_path=p, timestamp=sw["timestamp"], sensor2lidar_rotation=sw["sensor2lidar_rotation"],
                              sensor2lidar_translation=sw["sensor2lidar_translation"]))
        data = dict(pts_filename=key_path, sweeps=infos, timestamp=fr["timestamp"])
        data = L.LoadPointsFromFile(coord_type="LIDAR", load_dim=5, use_dim=5)(data)
        data = L.LoadPointsFromMultiSweeps(sweeps_num=10, use_dim=[0, 1, 2, 3, 4], test_mode=True)(data)
        loaded = data["points"].tensor.numpy().copy()
        data.update(gt_bboxes_3d=_Boxes(fr["gt_bboxes_3d"]), gt_labels_3d=fr["gt_labels_3d"].copy())
        if which == "main":
            data.update(img=[Image.fromarray(im) for im in fr["img"]], gt_bboxes=fr["gt_bboxes"].copy())
        t = transforms[which]
        t.set_epoch(epoch)
        calls = []
        np.random.seed(rng_seed)
        data = t(data)
        store[f"{case}.next_rand"] = np.float64(np.random.rand())
        pts = data["points"].tensor.numpy()
        none = int(pts.shape == loaded.shape and np.array_equal(pts, loaded))
        store[f"{case}.none"] = np.int64(none)
        store[f"{case}.calls"] = np.int64(len(calls))
        sampled_boxes = []
        for k, rec in enumerate(calls):
            thr_kinds.add(rec["thr"] == 0 if rec["thr"] is not None else None)
            m = check_call(rec, by_gid, gtp)
            contain_pairs += int((rec["bev"] & ~rec["bev_plain"]).sum())
            total_misses += m
            if len(rec["valid"]):
                sampled_boxes.append(np.stack([by_gid[g]["box3d_lidar"][:fr["gt_bboxes_3d"].shape[1]]
                                               for g in rec["valid"]]))
            store[f"{case}.{k}.name"] = np.int64(gc.CLASSES.index(rec["name"]))
            store[f"{case}.{k}.sampled"], store[f"{case}.{k}.valid"] = rec["sampled"], rec["valid"]
            store[f"{case}.{k}.bev"] = rec["bev"]
            if rec["c2d"] is not None:
                store[f"{case}.{k}.c2d"], store[f"{case}.{k}.thr"] = rec["c2d"], np.float64(rec["thr"])
        store[f"{case}.gt_bboxes_3d"] = data["gt_bboxes_3d"].tensor.numpy()
        store[f"{case}.gt_labels_3d"] = np.asarray(data["gt_labels_3d"])
        if which == "main":
            store[f"{case}.gt_bboxes"], store[f"{case}.gt_labels"] = data["gt_bboxes"], np.asarray(data.get(
                "gt_labels", np.zeros(0, np.int64)))
        if not none:
            boxes = np.concatenate(sampled_boxes)
            store[f"{case}.points"] = pts.copy()
            planes = np.concatenate([a[..., None] if a.ndim == 2 else a for a in ops.surface_equ_3d(
                ops.corner_to_surfaces_3d(ops.center_to_corner_box3d(boxes[:, :3], boxes[:, 3:6], boxes[:, 6],
                                                                     origin=(0.5, 0.5, 0), axis=2))[:, :, :3, :])], -1)
            store[f"{case}.planes"] = planes.astype(np.float32)
            # condition 1: no loaded point within 1e-3 m of a face of a sampled box
            p64 = planes.astype(np.float64)
            dist = (loaded[:, None, None, :3].astype(np.float64) * p64[None, :, :, :3]).sum(-1) + p64[None, :, :, 3]
            dist /= np.linalg.norm(p64[..., :3], axis=-1)[None]
            inside = (dist < 0).all(-1)
            risky = (np.abs(dist) < 1e-3).any(-1) & (dist < 1e-3).all(-1)      # per (point, box)
            assert not risky.any(), "a scene point within 1e-3 m of a face"
            assert inside.any(), "nothing to remove"
            n_obj = sum(by_gid[g]["num_points_in_gt"] for rec in calls for g in rec["valid"])
            assert pts.shape[0] == n_obj + loaded.shape[0] - int(inside.any(-1).sum())
            if fr["sweeps"]:
                raw = np.concatenate([fr["points"]] + [s["points"] for s in fr["sweeps"]])
                d_raw = (raw[:, None, None, :3].astype(np.float64) * p64[None, :, :, :3]).sum(-1) + p64[None, :, :, 3]
                before_pose = (d_raw < 0).all(-1).any(-1)
                assert (before_pose != inside.any(-1)).sum() > 20, "the pose does not change what is removed"
            if which == "main":
                store[f"{case}.img"] = np.stack([np.asarray(im) for im in data["img"]])
                assert any(not np.array_equal(a, b) for a, b in zip(store[f"{case}.img"], fr["img"]))
        if not none and case in ("f0", "sw"):
            # the crafted augmentation + range filter, through the reference's own point methods
            aug_pts = data["points"]
            aug_pts.tensor = aug_pts.tensor.clone()
            aug_pts.rotate(torch.from_numpy(gc.AUG["rot_mat_T"]))
            aug_pts.translate(np.asarray(gc.AUG["translation"]))
            aug_pts.scale(gc.AUG["scale"])
            aug_pts.flip("horizontal")
            out = T.PointsRangeFilter(point_cloud_range=gc.PC_RANGE)(dict(points=aug_pts))["points"].tensor.numpy()
            assert 0 < out.shape[0] < pts.shape[0]
            store[f"{case}.points_aug"] = out.copy()
        print(case, "calls", len(calls), "valid", sum(len(r["valid"]) for r in calls), "none", none,
              "points", pts.shape[0], "of", loaded.shape[0])

    expect_none = {"f2": 1, "stop": 1}
    for case, *_ in gc.CALLS:
        assert int(store[f"{case}.none"]) == expect_none.get(case, 0), case
    assert thr_kinds >= {True, False}, "both kinds of collision_thr draws are needed"
    assert contain_pairs > 0, "no pair collides by containment alone"
    assert len(set(resets)) >= 3, "BatchSampler must wrap round for several classes"
    print("containment-only pairs", contain_pairs, "| 2D overlaps the reference's corner order misses", total_misses)

    for k, (a, b) in enumerate(MODAL_SEEDS):
        np.random.seed(a)
        random.seed(b)
        out = T.ModalMask3D(mode="train")(dict(img=[None] * gc.NUM_VIEWS))["img_mask_idx"]
        store[f"modal.{k}"] = np.array(out, np.int64)
    store["modal.test"] = np.array(T.ModalMask3D(mode="test")(dict(img=[None] * gc.NUM_VIEWS))["img_mask_idx"])
    store["modal.seeds"] = np.array(MODAL_SEEDS)
    assert {tuple(store[f"modal.{k}"]) == (-1, -1, -1) for k in range(len(MODAL_SEEDS))} == {True, False}
    return store


def main():
    ref = install()
    seed = FIRST_SEED
    while True:
        try:
            with tempfile.TemporaryDirectory() as tmp:
                store = run(seed, ref, tmp)
            break
        except AssertionError as e:
            print("seed", seed, "rejected:", e)
            seed += 1
            if seed > FIRST_SEED + 40:
                raise
    path = os.path.join(HERE, "gt_paste_ref.npz")
    np.savez_compressed(path, **store)
    print("seed", seed, "wrote", path, os.path.getsize(path) // 1024, "KiB")
    assert os.path.getsize(path) < 600 * 1024


if __name__ == "__main__":
    main()
