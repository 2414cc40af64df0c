"""Host side of the multi-modal GT-paste: ObjectSampleV2 with MMDataBaseSamplerV2 (datasets/pipelines/
transforms_3d.py:1276-1382, dbsampler.py:13-195, :644-850, :902-998) and ModalMask3D (transforms_3d.py:1828-1862).

The split follows the reference's data flow.  What decides WHICH database objects get pasted stays here: the per-class
BatchSampler, the two database filters, the BEV / 2D collision tests (data_augment_utils.py:30-125,
box_np_ops.iou_jit) and the greedy acceptance loop, a few dozen boxes per sample, with np.random consumed in the
reference's order so that a seeded run samples the same objects.  Everything per point and per pixel goes to the
device: GTPasteSampler.sample() returns a plan that MultiSweepPointLoader(paste=...) (isf_assemble_points_paste) and
MultiViewImageLoader(paste=...) (isf_image_paste) execute inside the two batch calls.

Plans are drawn per sample BEFORE the batch calls, so the numpy RNG interleaves with the loaders' own draws as in the
reference only while no frame has more than sweeps_num sweeps (only then does the sweep choice draw nothing)."""
import os
import pickle
import random

import numpy as np

from . import _lib

IsfError = _lib.IsfError


# ======================================================================================================================
# geometry, in the reference's numpy expressions and dtypes (core/bbox/box_np_ops.py)
def corners_nd(dims, origin=0.5):
    """box_np_ops.py:49-80"""
    ndim = int(dims.shape[1])
    corners_norm = np.stack(np.unravel_index(np.arange(2 ** ndim), [2] * ndim), axis=1).astype(dims.dtype)
    if ndim == 2:
        corners_norm = corners_norm[[0, 1, 3, 2]]
    elif ndim == 3:
        corners_norm = corners_norm[[0, 1, 3, 2, 4, 5, 7, 6]]
    corners_norm = corners_norm - np.array(origin, dtype=dims.dtype)
    return dims.reshape([-1, 1, ndim]) * corners_norm.reshape([1, 2 ** ndim, ndim])


def rotation_2d(points, angles):
    """box_np_ops.py:83-97"""
    rot_sin, rot_cos = np.sin(angles), np.cos(angles)
    rot_mat_T = np.stack([[rot_cos, -rot_sin], [rot_sin, rot_cos]])
    return np.einsum("aij,jka->aik", points, rot_mat_T)


def center_to_corner_box2d(centers, dims, angles=None, origin=0.5):
    """box_np_ops.py:100-123"""
    corners = corners_nd(dims, origin=origin)
    if angles is not None:
        corners = rotation_2d(corners, angles)
    corners += centers.reshape([-1, 1, 2])
    return corners


def center_to_corner_box3d(centers, dims, angles=None, origin=(0.5, 0.5, 0)):
    """box_np_ops.py:206-235 with axis = 2 (rotation_3d_in_axis, :175-203), as points_in_rbbox calls it"""
    corners = corners_nd(dims, origin=origin)
    if angles is not None:
        rot_sin, rot_cos = np.sin(angles), np.cos(angles)
        ones, zeros = np.ones_like(rot_cos), np.zeros_like(rot_cos)
        rot_mat_T = np.stack([[rot_cos, -rot_sin, zeros], [rot_sin, rot_cos, zeros], [zeros, zeros, ones]])
        corners = np.einsum("aij,jka->aik", corners, rot_mat_T)
    corners += centers.reshape([-1, 1, 3])
    return corners


def corner_to_surfaces_3d(corners):
    """box_np_ops.py:404-423: [N, 8, 3] -> [N, 6, 4, 3], normals pointing inwards"""
    return np.array([
        [corners[:, 0], corners[:, 1], corners[:, 2], corners[:, 3]],
        [corners[:, 7], corners[:, 6], corners[:, 5], corners[:, 4]],
        [corners[:, 0], corners[:, 3], corners[:, 7], corners[:, 4]],
        [corners[:, 1], corners[:, 5], corners[:, 6], corners[:, 2]],
        [corners[:, 0], corners[:, 4], corners[:, 5], corners[:, 1]],
        [corners[:, 3], corners[:, 2], corners[:, 6], corners[:, 7]],
    ]).transpose([2, 0, 1, 3])


def surface_equ_3d(polygon_surfaces):
    """box_np_ops.py:694-715 -> (normal_vec [N, 6, 3], d [N, 6]) of a x + b y + c z + d = 0"""
    surface_vec = polygon_surfaces[:, :, :2, :] - polygon_surfaces[:, :, 1:3, :]
    normal_vec = np.cross(surface_vec[:, :, 0, :], surface_vec[:, :, 1, :])
    d = np.einsum("aij, aij->ai", normal_vec, polygon_surfaces[:, :, 0, :])
    return normal_vec, -d


def box_planes(boxes):
    """The six inward plane equations of points_in_rbbox(points, boxes) (box_np_ops.py:426-446, :778) -> [N, 6, 4] =
    (n0, n1, n2, d) in the boxes' dtype.  A point is inside a box when all six x n0 + y n1 + z n2 + d are < 0."""
    boxes = np.asarray(boxes)
    if boxes.shape[0] == 0:
        return np.zeros((0, 6, 4), boxes.dtype)
    corners = center_to_corner_box3d(boxes[:, :3], boxes[:, 3:6], boxes[:, 6], origin=(0.5, 0.5, 0))
    surfaces = corner_to_surfaces_3d(corners)
    normal_vec, d = surface_equ_3d(surfaces[:, :, :3, :])
    return np.concatenate([normal_vec, d[..., None]], axis=-1)


def box_collision_test(boxes, qboxes, clockwise=True):
    """data_augment_utils.py:30-125 for corner sets [N, 4, 2] x [K, 4, 2] -> bool [N, K], all pairs at once, each
    comparison in the reference's own expression.  It follows the COMPILED function: numba compares values for
    `ret[i, j] is True / False`, so a pair without crossing edges goes on to the containment test (:85-125) and a box
    lying wholly inside another collides.  (Run as plain Python on numpy bools those branches never fire.)"""
    boxes, qboxes = np.asarray(boxes), np.asarray(qboxes)
    N, K = boxes.shape[0], qboxes.shape[0]
    if N == 0 or K == 0:
        return np.zeros((N, K), dtype=np.bool_)
    nxt = np.array([1, 2, 3, 0])
    bs = np.concatenate([boxes.min(axis=1), boxes.max(axis=1)], axis=1)       # corner_to_standup_nd_jit
    qs = np.concatenate([qboxes.min(axis=1), qboxes.max(axis=1)], axis=1)
    iw = np.minimum(bs[:, None, 2], qs[None, :, 2]) - np.maximum(bs[:, None, 0], qs[None, :, 0])
    ih = np.minimum(bs[:, None, 3], qs[None, :, 3]) - np.maximum(bs[:, None, 1], qs[None, :, 1])
    near = (iw > 0) & (ih > 0)
    # edges: A -> B of box i (index k), C -> D of qbox j (index l); broadcast to [N, K, 4(k), 4(l)]
    A, B = boxes[:, None, :, None, :], boxes[:, nxt][:, None, :, None, :]
    C, D = qboxes[None, :, None, :, :], qboxes[:, nxt][None, :, None, :, :]
    acd = (D[..., 1] - A[..., 1]) * (C[..., 0] - A[..., 0]) > (C[..., 1] - A[..., 1]) * (D[..., 0] - A[..., 0])
    bcd = (D[..., 1] - B[..., 1]) * (C[..., 0] - B[..., 0]) > (C[..., 1] - B[..., 1]) * (D[..., 0] - B[..., 0])
    abc = (C[..., 1] - A[..., 1]) * (B[..., 0] - A[..., 0]) > (B[..., 1] - A[..., 1]) * (C[..., 0] - A[..., 0])
    abd = (D[..., 1] - A[..., 1]) * (B[..., 0] - A[..., 0]) > (B[..., 1] - A[..., 1]) * (D[..., 0] - A[..., 0])
    crossing = ((acd != bcd) & (abc != abd)).any(axis=(2, 3))

    def holds(outer, inner):
        """every corner l of inner[j] strictly inside outer[i]: [len(outer), len(inner)]"""
        vec = outer - outer[:, nxt]
        if clockwise:
            vec = -vec
        vec = vec[:, None, :, None, :]                                        # [i, 1, k, 1, 2]
        corner = outer[:, None, :, None, :]                                   # [i, 1, k, 1, 2]
        point = inner[None, :, None, :, :]                                    # [1, j, 1, l, 2]
        cross = vec[..., 1] * (corner[..., 0] - point[..., 0])
        cross = cross - vec[..., 0] * (corner[..., 1] - point[..., 1])
        return ~(cross >= 0).any(axis=(2, 3))

    box_holds_q = holds(boxes, qboxes)
    q_holds_box = holds(qboxes, boxes).T
    return near & (crossing | box_holds_q | q_holds_box)


def iof(boxes, query_boxes):
    """box_np_ops.iou_jit(boxes, query_boxes, 'iof') (box_np_ops.py:568-606, eps = 0): intersection over the area of
    boxes[n] -> [N, K] in the boxes' dtype"""
    boxes, query_boxes = np.asarray(boxes), np.asarray(query_boxes)
    iw = np.minimum(boxes[:, None, 2], query_boxes[None, :, 2]) - np.maximum(boxes[:, None, 0], query_boxes[None, :, 0])
    ih = np.minimum(boxes[:, None, 3], query_boxes[None, :, 3]) - np.maximum(boxes[:, None, 1], query_boxes[None, :, 1])
    ua = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]))[:, None]
    hit = (iw > 0) & (ih > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        val = iw * ih / ua
    return np.where(hit, val, np.zeros((), boxes.dtype)).astype(boxes.dtype)


def resolve_slice(start, stop, size):
    """numpy's a[start:stop] on an axis of `size` as a concrete [begin, end): slices clip, negative bounds wrap"""
    begin, end, _ = slice(int(start), int(stop)).indices(int(size))
    return begin, max(end, begin)


# ======================================================================================================================
class BatchSampler:
    """dbsampler.py:13-77: a shuffled round robin over one class's database entries.  The constructor shuffles, and
    the indices are shuffled again whenever _idx + num >= len (the tail is handed out first)."""

    def __init__(self, sampled_list, name=None, shuffle=True):
        self._sampled_list = sampled_list
        self._indices = np.arange(len(sampled_list))
        if shuffle:
            np.random.shuffle(self._indices)
        self._idx = 0
        self._example_num = len(sampled_list)
        self._name = name
        self._shuffle = shuffle

    def _sample(self, num):
        if self._idx + num >= self._example_num:
            ret = self._indices[self._idx:].copy()
            self._reset()
        else:
            ret = self._indices[self._idx:self._idx + num]
            self._idx += num
        return ret

    def _reset(self):
        assert self._name is not None
        if self._shuffle:
            np.random.shuffle(self._indices)
        self._idx = 0

    def sample(self, num):
        return [self._sampled_list[i] for i in self._sample(num)]


class GTPastePlan:
    """What one ObjectSampleV2 call decided, for the two batch loaders to execute.
    gt_bboxes_3d float32 [G + S, 7 | 9], gt_labels_3d int64 [G + S], gt_bboxes [G + S, 4] (None without sample_2d):
        the concatenated ground truth (transforms_3d.py:1353-1379);
    objects: the S valid objects in the order sampled, each dict(points = path or float32 [n, 5] array,
        translation = float32 [3] (box3d_lidar[:3]), patch = uint8 [h, w, 3] RGB or None, name, index);
    planes float32 [S, 6, 4]: the removal boxes' inward plane equations;
    image_ops: ordered list of dict(view, kind = 'mix' | 'patch', rows (r0, r1), cols (c0, c1)[, object, mask_rows,
        mask_cols]) with every rectangle resolved against its view; empty without sample_2d;
    mixup: the sampler's."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _find_transform(pipeline, name):
    for t in pipeline:
        if t.get("type") == name:
            return t
        if "transforms" in t:
            found = _find_transform(t["transforms"], name)
            if found is not None:
                return found
    return None


class GTPasteSampler:
    """ObjectSampleV2 + its db_sampler.  Constructor arguments carry the reference's names (MMDataBaseSamplerV2:
    info_path, data_root, rate, prepare, sample_groups, classes, check_2D_collision, collision_thr,
    collision_in_classes, depth_consistent, blending_type, mixup, img_num, points_loader; ObjectSampleV2: sample_2d,
    stop_epoch).  db_infos: the database dict (class name -> list of dict(name, path, box3d_lidar, box2d_camera,
    num_points_in_gt, difficulty)); None reads the pickle at info_path.  An entry's `path` may be a float32 [n, 5]
    array in place of a file name, and a `patch` key may hold its uint8 [h, w, 3] RGB image patch in place of
    path + '.png'.

    With sample_2d=False the reference's ObjectSampleV2 only works over the plain DataBaseSampler (sample_all without
    images, dbsampler.py:197-328: BEV collisions only, always across classes); that is what sample_2d=False follows."""

    def __init__(self, info_path=None, data_root=None, rate=1.0, prepare=None, sample_groups=None, classes=None,
                 check_2D_collision=False, collision_thr=0, collision_in_classes=False, depth_consistent=False,
                 blending_type=None, mixup=1.0, img_num=1, points_loader=None, sample_2d=False, stop_epoch=None,
                 db_infos=None):
        if blending_type:
            raise IsfError(f"blending_type={blending_type!r}: the V2 paste path (paste_obj_v2) never blends; only None "
                           "is built")
        if classes is None or sample_groups is None:
            raise IsfError("GTPasteSampler needs `classes` and `sample_groups`")
        if points_loader is not None and (points_loader.get("load_dim", 5) != 5
                                          or list(points_loader.get("use_dim", range(5))) != [0, 1, 2, 3, 4]):
            raise IsfError("database objects are float32 [n, 5] files (load_dim=5, use_dim=[0..4])")
        self.info_path, self.data_root, self.rate = info_path, data_root, rate
        self.prepare, self.classes = dict(prepare or {}), list(classes)
        self.cat2label = {name: i for i, name in enumerate(self.classes)}
        self.label2cat = {i: name for i, name in enumerate(self.classes)}
        self.check_2D_collision, self.collision_thr = check_2D_collision, collision_thr
        self.collision_in_classes, self.depth_consistent = collision_in_classes, depth_consistent
        self.blending_type, self.mixup, self.img_num = blending_type, mixup, img_num
        self.points_loader = points_loader
        self.sample_2d, self.stop_epoch, self.epoch = bool(sample_2d), stop_epoch, -1
        if db_infos is None:
            if info_path is None:
                raise IsfError("GTPasteSampler needs db_infos or info_path")
            with open(info_path, "rb") as f:
                db_infos = pickle.load(f)
        for prep_func, val in self.prepare.items():
            db_infos = getattr(self, prep_func)(db_infos, val)
        self.db_infos = db_infos
        self.sample_classes = list(sample_groups.keys())
        self.sample_max_nums = [int(v) for v in sample_groups.values()]
        self.sampler_dict = {k: BatchSampler(v, k, shuffle=True) for k, v in self.db_infos.items()}
        self.last_debug = None      # per sample_class call: (class, sampled indices, collision matrices, valid mask)

    @classmethod
    def from_config(cls, config, db_infos=None):
        """config: path of the unmodified configs/isfusion/isfusion_0075voxel.py, its variable dict, or the
        (train_pipeline, test_pipeline) lists alone -> the sampler of the train pipeline's ObjectSampleV2 entry"""
        if isinstance(config, str):
            from . import registry
            config = registry.load_config(config)
        pipeline = config["train_pipeline"] if isinstance(config, dict) else config[0]
        entry = _find_transform(pipeline, "ObjectSampleV2")
        if entry is None:
            raise KeyError("the train pipeline has no ObjectSampleV2 entry")
        kw = {k: v for k, v in entry["db_sampler"].items() if k != "type"}
        return cls(sample_2d=entry.get("sample_2d", False), stop_epoch=entry.get("stop_epoch"), db_infos=db_infos, **kw)

    def set_epoch(self, epoch):
        self.epoch = epoch

    # ------------------------------------------------------------------------------------------------ database
    @staticmethod
    def filter_by_difficulty(db_infos, removed_difficulty):
        """dbsampler.py:156-173"""
        return {key: [info for info in dinfos if info["difficulty"] not in removed_difficulty]
                for key, dinfos in db_infos.items()}

    @staticmethod
    def filter_by_min_points(db_infos, min_gt_points_dict):
        """dbsampler.py:175-195"""
        for name, min_num in min_gt_points_dict.items():
            min_num = int(min_num)
            if min_num > 0:
                db_infos[name] = [info for info in db_infos[name] if info["num_points_in_gt"] >= min_num]
        return db_infos

    def _points_source(self, info):
        path = info["path"]
        if isinstance(path, (str, bytes)):
            return os.path.join(self.data_root, path) if self.data_root else path
        return path

    def _patch(self, info):
        """the object's image patch, uint8 [h, w, 3] RGB (the reference loads BGR and swaps, dbsampler.py:919)"""
        if info.get("patch") is not None:
            patch = np.asarray(info["patch"])
        else:
            from PIL import Image
            with Image.open(self._points_source(info) + ".png") as im:
                patch = np.asarray(im.convert("RGB"))
        if patch.dtype != np.uint8 or patch.ndim != 3 or patch.shape[2] != 3:
            raise IsfError(f"image patches are uint8 [h, w, 3]; got {patch.dtype} {patch.shape}")
        return np.ascontiguousarray(patch)

    # ------------------------------------------------------------------------------------------------ sampling
    def _draw_collision_thr(self):
        """dbsampler.py:953-965"""
        thr = self.collision_thr
        if isinstance(thr, (float, int)):
            return thr
        if isinstance(thr, list):
            return np.random.choice(thr)
        if isinstance(thr, dict):
            mode = thr.get("mode", "value")
            if mode == "value":
                return np.random.choice(thr["thr_range"])
            if mode == "range":
                return np.random.uniform(thr["thr_range"][0], thr["thr_range"][1])
        raise IsfError(f"collision_thr={thr!r} is none of the reference's forms")

    def sample_class(self, name, num, gt_bboxes_3d, gt_bboxes_2d, check_2d):
        """sample_class_v2 (dbsampler.py:930-998; :291-328 without the 2D test) -> the valid samples"""
        indices = self.sampler_dict[name]._sample(num)
        sampled = [self.db_infos[name][i] for i in indices]
        num_gt, num_sampled = gt_bboxes_3d.shape[0], len(sampled)
        gt_bv = center_to_corner_box2d(gt_bboxes_3d[:, 0:2], gt_bboxes_3d[:, 3:5], gt_bboxes_3d[:, 6])
        sp_boxes = np.stack([i["box3d_lidar"] for i in sampled], axis=0)
        sp_bv = center_to_corner_box2d(sp_boxes[:, 0:2], sp_boxes[:, 3:5], sp_boxes[:, 6])
        total_bv = np.concatenate([gt_bv, sp_bv], axis=0)
        coll_bev = box_collision_test(total_bv, total_bv)
        coll_mat, coll_2d, thr = coll_bev.copy(), None, None
        if check_2d:
            sp_boxes_2d = np.stack([i["box2d_camera"] for i in sampled], axis=0)
            if gt_bboxes_2d.shape[0] == 0:
                total_2d = sp_boxes_2d
            else:
                total_2d = np.concatenate([gt_bboxes_2d, sp_boxes_2d], axis=0)
            thr = self._draw_collision_thr()
            if thr == 0:
                x1y1, x2y2 = total_2d[:, :2], total_2d[:, 2:4]
                x1y2 = np.stack([total_2d[:, 0], total_2d[:, 3]], axis=-1)
                x2y1 = np.stack([total_2d[:, 2], total_2d[:, 1]], axis=-1)
                corners = np.stack([x1y1, x2y1, x1y2, x2y2], axis=1)
                coll_2d = box_collision_test(corners, corners)
            else:
                coll_2d = iof(total_2d, total_2d) > thr
            coll_mat = coll_mat | coll_2d
        diag = np.arange(total_bv.shape[0])
        coll_mat[diag, diag] = False
        valid = np.zeros(num_sampled, dtype=bool)
        for i in range(num_gt, num_gt + num_sampled):       # the greedy acceptance loop, :987-996
            if coll_mat[i].any():
                coll_mat[i] = False
                coll_mat[:, i] = False
            else:
                valid[i - num_gt] = True
        self.last_debug.append(dict(name=name, indices=np.array(indices), coll_bev=coll_bev, coll_2d=coll_2d,
                                    collision_thr=thr, valid=valid))
        return [(int(indices[k]), sampled[k]) for k in range(num_sampled) if valid[k]]

    def sample(self, result):
        """ObjectSampleV2.__call__ without its per-point and per-pixel work.  result: dict with the reference's keys
        gt_bboxes_3d ([G, 7 | 9] array, or an object with .tensor), gt_labels_3d [G] and, with sample_2d, gt_bboxes
        [G, 5] (x1, y1, x2, y2, camera index) and img (the views; only their shapes are read).  The ground-truth keys
        of `result` are updated as the reference does.  -> GTPastePlan, or None past stop_epoch or when nothing is
        valid (gt_bboxes is still cut to [:, :4] and gt_labels still set then, transforms_3d.py:1374-1376)."""
        self.last_debug = []
        if self.stop_epoch is not None and self.epoch >= self.stop_epoch:
            return None
        boxes = result["gt_bboxes_3d"]
        gt_bboxes_3d = boxes.tensor.numpy() if hasattr(boxes, "tensor") else np.asarray(boxes, dtype=np.float32)
        gt_labels_3d = np.asarray(result["gt_labels_3d"])
        gt_bboxes_2d = np.asarray(result["gt_bboxes"]) if self.sample_2d else None

        sample_num_per_class = []
        for class_name, max_sample_num in zip(self.sample_classes, self.sample_max_nums):
            class_label = self.cat2label[class_name]
            sampled_num = int(max_sample_num - np.sum([n == class_label for n in gt_labels_3d]))
            sample_num_per_class.append(np.round(self.rate * sampled_num).astype(np.int64))

        sampled, sampled_3d, sampled_2d = [], [], []
        avoid_3d, avoid_2d = gt_bboxes_3d, gt_bboxes_2d
        accumulate = self.collision_in_classes or not self.sample_2d
        for class_name, sampled_num in zip(self.sample_classes, sample_num_per_class):
            if sampled_num > 0:
                sampled_cls = self.sample_class(class_name, sampled_num, avoid_3d, avoid_2d,
                                                self.sample_2d and self.check_2D_collision)
                sampled += sampled_cls
                if len(sampled_cls) > 0:
                    box_3d = np.stack([s["box3d_lidar"] for _, s in sampled_cls], axis=0)
                    sampled_3d.append(box_3d)
                    if self.sample_2d:
                        box_2d = np.stack([s["box2d_camera"] for _, s in sampled_cls], axis=0)
                        sampled_2d.append(box_2d)
                    if accumulate:
                        avoid_3d = np.concatenate([avoid_3d, box_3d], axis=0)
                        if self.sample_2d:
                            avoid_2d = np.concatenate([avoid_2d, box_2d], axis=0)

        plan = None
        if len(sampled) > 0:
            sampled_3d = np.concatenate(sampled_3d, axis=0)
            sampled_labels = np.array([self.cat2label[s["name"]] for _, s in sampled], dtype=np.int64)
            objects = [dict(points=self._points_source(s), translation=np.asarray(s["box3d_lidar"][:3], np.float32),
                            patch=None, name=s["name"], index=i) for i, s in sampled]
            image_ops = []
            if self.sample_2d:
                sampled_2d = np.concatenate(sampled_2d, axis=0)
                image_ops = self._image_ops(result["img"], gt_bboxes_3d, gt_bboxes_2d, sampled_3d, sampled_2d,
                                            [s for _, s in sampled], objects)
                if gt_bboxes_2d.shape[0] == 0:
                    gt_bboxes_2d = sampled_2d
                else:
                    gt_bboxes_2d = np.concatenate([gt_bboxes_2d, sampled_2d]).astype(np.float32)
            gt_labels_3d = np.concatenate([gt_labels_3d, sampled_labels], axis=0)
            all_3d = np.concatenate([gt_bboxes_3d, sampled_3d]).astype(np.float32)     # new_box: a float32 tensor
            plan = GTPastePlan(gt_bboxes_3d=all_3d, gt_labels_3d=gt_labels_3d.astype(np.int64), gt_bboxes=None,
                               gt_labels=None, objects=objects,
                               planes=np.ascontiguousarray(box_planes(sampled_3d), dtype=np.float32),
                               image_ops=image_ops, mixup=self.mixup, sample_2d=self.sample_2d,
                               sampled_gt_bboxes_3d=sampled_3d)
            gt_bboxes_3d = all_3d
        if self.sample_2d:
            result["gt_bboxes"] = gt_bboxes_2d[:, :4]
            result["gt_labels"] = gt_labels_3d.astype(np.int64)
            if plan is not None:
                plan.gt_bboxes, plan.gt_labels = result["gt_bboxes"], result["gt_labels"]
        if plan is not None or not hasattr(boxes, "tensor"):
            result["gt_bboxes_3d"] = gt_bboxes_3d
        result["gt_labels_3d"] = gt_labels_3d.astype(np.int64)
        return plan

    # ------------------------------------------------------------------------------------------------ image side
    def _image_ops(self, imgs, gt_bboxes_3d, gt_bboxes_2d, sampled_3d, sampled_2d, sampled, objects):
        """The far-to-near loop of sample_all (dbsampler.py:748-831) as a list of rectangle operations.  Step idx
        handles object `position of idx in argsort(-x)` -- the inverse permutation, as the reference does.  Real
        ground truth indexes rows by x1:x2 and columns by y1:y2 (:814).  Where numpy would raise because a patch and
        its region differ in shape, this raises before anything is launched."""
        shapes = [(im.size[1], im.size[0]) if hasattr(im, "mode") else np.asarray(im).shape[:2] for im in imgs]
        num_origin = gt_bboxes_2d.shape[0]
        if num_origin == 0:
            all_3d, boxes_2d = sampled_3d, sampled_2d
        else:
            all_3d = np.concatenate([gt_bboxes_3d, sampled_3d], axis=0)
            boxes_2d = np.concatenate([gt_bboxes_2d, sampled_2d], axis=0)
        camera, all_2d = boxes_2d[:, -1], boxes_2d[:, :4]
        order = np.argsort(-all_3d[:, 0])
        ops = []
        for idx in range(all_3d.shape[0]):
            inds = np.where(order == idx)[0][0]
            view = int(camera[inds])
            if view >= self.img_num:
                continue
            if not 0 <= view < len(shapes):
                raise IsfError(f"object on camera {view}, the sample has {len(shapes)} views")
            H, W = shapes[view]
            if inds < num_origin:                                   # real GT: mix the original pixels back
                x1, y1, x2, y2 = [int(v) for v in all_2d[inds]]
                rows, cols = resolve_slice(x1, x2, H), resolve_slice(y1, y2, W)
                if rows[1] > rows[0] and cols[1] > cols[0]:
                    ops.append(dict(view=view, kind="mix", rows=rows, cols=cols))
                continue
            k = int(inds - num_origin)
            if objects[k]["patch"] is None:
                objects[k]["patch"] = self._patch(sampled[k])
            patch = objects[k]["patch"]
            x1, y1, x2, y2 = [int(v) for v in all_2d[inds].astype(np.int32)]
            w = max(min(x2, W - 1) - x1 + 1, 1)                     # paste_obj_v2, :906-908
            h = max(min(y2, H - 1) - y1 + 1, 1)
            ph, pw = min(h, patch.shape[0]), min(w, patch.shape[1])  # obj_img[:h, :w]
            rows, cols = resolve_slice(y1, y1 + h, H), resolve_slice(x1, x1 + w, W)
            region = (rows[1] - rows[0], cols[1] - cols[0])
            if region != (h, w) or (ph, pw) != (h, w):
                raise IsfError(f"GT-paste: object {k} ({objects[k]['name']}) has a patch of {patch.shape[:2]} for the "
                               f"{h} x {w} mask over an image region of {region}: the reference's paste_obj_v2 cannot "
                               "broadcast these (or broadcasts a one-pixel axis, which is not built)")
            margin_h, margin_w = int(0.05 * h), int(0.05 * w)
            ops.append(dict(view=view, kind="patch", rows=rows, cols=cols, object=k,
                            mask_rows=(rows[0] + margin_h, rows[0] + h - margin_h),
                            mask_cols=(cols[0] + margin_w, cols[0] + w - margin_w)))
        return ops


def draw_modal_mask(num_views, mode="test", dataset_type="NuScenesDataset"):
    """ModalMask3D.__call__ (transforms_3d.py:1838-1862) -> img_mask_idx: one np.random.rand() draw, then Python's
    random.sample of 3 (nuScenes) or 2 views when it is above 0.5, else a list of -1"""
    if mode == "test":
        return [0]
    seed = np.random.rand()
    count = 3 if dataset_type == "NuScenesDataset" else 2
    if seed > 0.5:
        return random.sample(range(num_views), count)
    return [-1] * count
