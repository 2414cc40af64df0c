"""Host side of the input pre-pass.  First half: the point path of the reference's data pipeline --
LoadPointsFromFile + LoadPointsFromMultiSweeps (datasets/pipelines/loading.py:1345-1516, :735-907), the point side of
GlobalRotScaleTransV2 / RandomFlip3DV2 (datasets/pipelines/transforms_3d.py:1871-1915, :1163-1204),
PointsRangeFilter (:2002-2037) and PointShuffle (:1918-1943) -- for a whole batch on the GPU.

The host only reads the sweep files into ONE pinned buffer (no per-point work on the CPU) and fills one descriptor per
file; libisf_hip.so (isf_assemble_points) applies time column / remove_close / sensor pose / augmentation / range
filter and compacts per sample in the reference's order.  No CPU fallback: without a GPU this raises.

Second half: the camera path of the same pipeline -- ImageAug3D + ImageNormalize (transforms_3d.py:45-145, :24-43) for
every view of a batch (MultiViewImageLoader over isf_image_prepass), with the img_aug_matrix it returns -- and the
ground-truth side of the LiDAR augmentation draw: lidar_aug_matrix and augment_gt_boxes."""
import ctypes
import functools
import math

import numpy as np
import torch

from . import _lib

POINT_DIM = 5


def rotation_matrix_T(angle):
    """rot_mat_T of BasePoints.rotate(angle) about the z axis (core/points/base_points.py:156-173, float32 sin / cos as
    the reference computes them)."""
    a = torch.tensor(float(angle), dtype=torch.float32)
    s, c = torch.sin(a), torch.cos(a)
    return torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=torch.float32).T.contiguous().numpy()


def draw_train_aug(resize_lim=(0.9, 1.1), rot_lim=(-0.78539816, 0.78539816), trans_lim=0.5, flip=True):
    """One draw of the training augmentation in the reference's numpy RNG order: GlobalRotScaleTransV2 (scale, theta,
    3 x normal; transforms_3d.py:1882-1884; points are rotated by -theta, :1888) then RandomFlip3DV2 (two
    np.random.choice draws, :1167-1168)."""
    scale = np.random.uniform(*resize_lim)
    theta = np.random.uniform(*rot_lim)
    translation = np.array([np.random.normal(0, trans_lim) for _ in range(3)])
    fh = fv = 0
    if flip:
        fh, fv = int(np.random.choice([0, 1])), int(np.random.choice([0, 1]))
    return dict(rot_mat_T=rotation_matrix_T(-theta), translation=translation, scale=scale,
                flip_horizontal=bool(fh), flip_vertical=bool(fv), theta=theta)


def flip_tta_views(points, meta, flip=True, pcd_horizontal_flip=True, pcd_vertical_flip=True, pts_scale_ratio=(1.0,)):
    """The views of MultiScaleFlipAug3D (datasets/pipelines/test_time_aug.py:66-111) through the test branch of
    RandomFlip3DV2 (transforms_3d.py:1188-1204), for one frame.  points: [N, >= 3] tensor or array; meta: its dict
    (lidar_aug_matrix 4 x 4, identity when absent).  Views in the reference's order: for each pts_scale_ratio, for
    horizontal in ([False, True] if flip and pcd_horizontal_flip else [False]), for vertical in (likewise).  A
    horizontal flip negates y, a vertical one x; lidar_aug_matrix[:3, :] = R @ lidar_aug_matrix[:3, :] with R = V @ H;
    each view's meta gets pcd_horizontal_flip, pcd_vertical_flip, pcd_scale_factor and transformation_3d_flow.  As in
    the shipped test pipeline (GlobalRotScaleTransV2 with is_train=False), the points are not scaled: pcd_scale_factor
    only scales the boxes back in the merge.  -> (list of points, list of metas)."""
    if not flip and (pcd_horizontal_flip or pcd_vertical_flip):
        pcd_horizontal_flip = pcd_vertical_flip = False     # MultiScaleFlipAug3D: no flip views without `flip`
    if isinstance(pts_scale_ratio, (int, float)):
        pts_scale_ratio = [pts_scale_ratio]
    hs = [False, True] if pcd_horizontal_flip else [False]
    vs = [False, True] if pcd_vertical_flip else [False]
    lam0 = np.asarray(meta.get("lidar_aug_matrix", np.eye(4, dtype=np.float32)))
    out_pts, out_metas = [], []
    for scale in pts_scale_ratio:
        for h in hs:
            for v in vs:
                p = points.clone() if isinstance(points, torch.Tensor) else np.array(points, copy=True)
                m = dict(meta)
                flow = list(meta.get("transformation_3d_flow", []))
                rotation = np.eye(3)
                if h:
                    rotation = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1]]) @ rotation
                    p[:, 1] = -p[:, 1]
                    flow.append("HF")
                if v:
                    rotation = np.array([[-1, 0, 0], [0, 1, 0], [0, 0, 1]]) @ rotation
                    p[:, 0] = -p[:, 0]
                    flow.append("VF")
                lam = lam0.copy()
                lam[:3, :] = rotation @ lam[:3, :]
                m.update(lidar_aug_matrix=lam, pcd_horizontal_flip=h, pcd_vertical_flip=v, pcd_scale_factor=scale,
                         transformation_3d_flow=flow, flip=bool(flip))
                out_pts.append(p)
                out_metas.append(m)
    return out_pts, out_metas


class MultiSweepPointLoader:
    """Batch replacement for the LoadPointsFromFile -> LoadPointsFromMultiSweeps -> [GlobalRotScaleTransV2 ->
    RandomFlip3DV2] -> PointsRangeFilter [-> PointShuffle] chain of configs/isfusion/isfusion_0075voxel.py:238-352.
    Constructor arguments carry the reference's names (LoadPointsFromMultiSweeps: sweeps_num, remove_close,
    test_mode; PointsRangeFilter: point_cloud_range)."""

    def __init__(self, sweeps_num=10, remove_close=False, test_mode=False, point_cloud_range=None, close_radius=1.0,
                 shuffle=False, device="cuda"):
        self.sweeps_num, self.remove_close, self.test_mode = sweeps_num, remove_close, test_mode
        self.point_cloud_range = None if point_cloud_range is None else [float(v) for v in point_cloud_range]
        self.close_radius, self.shuffle = float(close_radius), shuffle
        self.device = torch.device(device)
        self._pinned = None

    # ------------------------------------------------------------------------------------------------ host side
    @staticmethod
    def _read(src):
        """a sweep file path (flat float32, loading.py:797) or an already loaded array -> flat float32 view"""
        if isinstance(src, (str, bytes)):
            return np.fromfile(src, dtype=np.float32)
        return np.ascontiguousarray(src, dtype=np.float32).reshape(-1)

    def _choose(self, num):
        """sweep choice of loading.py:871-877"""
        if num <= self.sweeps_num:
            return np.arange(num)
        if self.test_mode:
            return np.arange(self.sweeps_num)
        return np.random.choice(num, self.sweeps_num, replace=False)

    def _stage(self, arrays):
        total = sum(a.size for a in arrays)
        if self._pinned is None or self._pinned.numel() < total:
            self._pinned = torch.empty(max(total, 1), dtype=torch.float32).pin_memory()
        host = self._pinned[:total]
        view, at = host.numpy(), 0
        for a in arrays:
            view[at:at + a.size] = a
            at += a.size
        return host

    def __call__(self, results_list, aug=None, paste=None):
        """results_list: one dict per sample with the reference's keys -- 'pts_filename' (path or float32 [P, 5]
        array), 'timestamp' (s), 'sweeps': [dict(data_path (path or array), timestamp (us), sensor2lidar_rotation,
        sensor2lidar_translation)].  aug: None or one dict per sample (draw_train_aug).  paste: None or per sample a
        gt_paste.GTPastePlan or None (ObjectSampleV2, transforms_3d.py:1348-1361: the plan's objects come first, and
        frame points inside a sampled box are dropped after the sensor pose; isf_assemble_points_paste).
        -> list of float32 [N_b, 5] device tensors (views of one buffer), in the reference's point order."""
        if self.device.type != "cuda":
            raise _lib.IsfError("MultiSweepPointLoader runs on the GPU only (isf_assemble_points); no CPU fallback")
        lib = _lib.load()
        B = len(results_list)
        arrays, descs, row = [], [], 0

        if paste is not None and len(paste) != B:
            raise _lib.IsfError(f"paste holds {len(paste)} plans for {B} samples")

        def add(arr, sample, is_sweep, lag=0.0, rot=None, trans=None):
            nonlocal row
            assert arr.size % POINT_DIM == 0, "sweep files hold float32 [P, 5]"
            d = _lib.Sweep()
            d.first_point, d.num_points, d.sample, d.is_sweep = row, arr.size // POINT_DIM, sample, int(is_sweep)
            d.remove_close, d.close_radius = int(self.remove_close and is_sweep == 1), self.close_radius
            d.time_lag = float(np.float32(lag))
            r = np.eye(3) if rot is None else np.asarray(rot, dtype=np.float64)
            t = np.zeros(3) if trans is None else np.asarray(trans, dtype=np.float64)
            d.rotation = (ctypes.c_double * 9)(*r.reshape(-1))
            d.translation = (ctypes.c_double * 3)(*t.reshape(-1))
            arrays.append(arr)
            descs.append(d)
            row += d.num_points

        planes, box_offsets = [], [0]
        for b, res in enumerate(results_list):
            plan = paste[b] if paste is not None else None
            if plan is not None:
                for obj in plan.objects:      # the float32 translation travels in the descriptor's float64 slot
                    add(self._read(obj["points"]), b, _lib.SWEEP_PASTED, trans=np.asarray(obj["translation"], np.float32))
                planes.append(np.asarray(plan.planes, np.float32).reshape(-1, 24))
            box_offsets.append(box_offsets[-1] + (0 if plan is None else planes[-1].shape[0]))
            add(self._read(res["pts_filename"]), b, False)
            sweeps = res.get("sweeps", [])
            for i in self._choose(len(sweeps)):
                sw = sweeps[int(i)]
                add(self._read(sw["data_path"]), b, True, res["timestamp"] - sw["timestamp"] / 1e6,
                    sw["sensor2lidar_rotation"], sw["sensor2lidar_translation"])
        raw = self._stage(arrays).to(self.device, non_blocking=True)
        out = torch.empty((max(row, 1), POINT_DIM), dtype=torch.float32, device=self.device)
        offsets = torch.empty((B + 1,), dtype=torch.int32, device=self.device)
        host_offsets = (ctypes.c_int32 * (B + 1))()
        sw_arr = (_lib.Sweep * len(descs))(*descs)
        aug_arr = None
        if aug is not None:
            aug_arr = (_lib.PointAug * B)()
            for b, a in enumerate(aug):
                if not a:
                    continue
                g = aug_arr[b]
                g.enabled = 1
                g.rot_mat_T = (ctypes.c_float * 9)(*np.asarray(a.get("rot_mat_T", np.eye(3)), np.float32).reshape(-1))
                g.translation = (ctypes.c_float * 3)(*np.asarray(a.get("translation", np.zeros(3)), np.float32))
                g.scale = float(a.get("scale", 1.0))
                g.flip_horizontal, g.flip_vertical = int(a.get("flip_horizontal", 0)), int(a.get("flip_vertical", 0))
        rng = None
        if self.point_cloud_range is not None:
            rng = (ctypes.c_float * 6)(*self.point_cloud_range)
        with torch.cuda.device(self.device):
            if paste is None:
                _lib.check(lib.isf_assemble_points(_lib.ptr(raw), sw_arr, len(descs), B, aug_arr, rng, _lib.ptr(out),
                                                   _lib.ptr(offsets), host_offsets, _lib.stream()),
                           "isf_assemble_points")
            else:
                flat = np.ascontiguousarray(np.concatenate(planes) if planes else np.zeros((0, 24), np.float32))
                _lib.check(lib.isf_assemble_points_paste(
                    _lib.ptr(raw), sw_arr, len(descs), B, aug_arr, rng,
                    flat.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), (ctypes.c_int32 * (B + 1))(*box_offsets),
                    _lib.ptr(out), _lib.ptr(offsets), host_offsets, _lib.stream()), "isf_assemble_points_paste")
        pts = [out[host_offsets[b]:host_offsets[b + 1]] for b in range(B)]
        if self.shuffle:        # PointShuffle: BasePoints.shuffle = tensor[randperm] (base_points.py, torch RNG)
            pts = [p[torch.randperm(p.shape[0], device=p.device)] for p in pts]
        return pts


# ======================================================================================================================
# ground-truth side of draw_train_aug()
def _box_rot_mat_T(boxes, theta):
    """rot_mat_T of LiDARInstance3DBoxes.rotate(angle) (core/bbox/structures/lidar_box3d.py:132-142): NOT the transpose
    BasePoints.rotate builds -- boxes turn by +theta where the points turn by -theta"""
    angle = boxes.new_tensor(theta)
    s, c = torch.sin(angle), torch.cos(angle)
    return angle, boxes.new_tensor([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def _flip_rotation(aug):
    rotation = np.eye(3)
    if aug.get("flip_horizontal"):
        rotation = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1]]) @ rotation
    if aug.get("flip_vertical"):
        rotation = np.array([[-1, 0, 0], [0, 1, 0], [0, 0, 1]]) @ rotation
    return rotation


def lidar_aug_matrix(aug):
    """The float32 [4, 4] lidar_aug_matrix that goes with one draw_train_aug() dict: GlobalRotScaleTransV2
    (transforms_3d.py:1879-1899: rotation = eye(3) @ gt_boxes.rotate(theta), transform[:3, :3] = rotation.T * scale,
    transform[:3, 3] = translation * scale) then RandomFlip3DV2 (:1170-1203: transform[:3, :] = (V @ H) @ transform[:3, :]).
    Point-to-Grid undoes the augmentation with its inverse before it projects pillars into the images."""
    transform = np.eye(4).astype(np.float32)
    _, rot_mat_T = _box_rot_mat_T(torch.zeros(1, dtype=torch.float32), aug["theta"])
    rotation = np.eye(3) @ rot_mat_T.numpy()
    transform[:3, :3] = rotation.T * aug["scale"]
    transform[:3, 3] = np.asarray(aug["translation"]) * aug["scale"]
    transform[:3, :] = _flip_rotation(aug) @ transform[:3, :]
    return transform


def augment_gt_boxes(boxes, labels, aug, point_cloud_range, num_classes):
    """The ground-truth side of one draw_train_aug() dict, in the reference's float32 torch ops and order:
    LiDARInstance3DBoxes.rotate(theta) / translate / scale (lidar_box3d.py:117-169, base_box3d.py:150-158, :216-223) of
    GlobalRotScaleTransV2, flip('horizontal') / flip('vertical') (lidar_box3d.py:171-192) of RandomFlip3DV2,
    ObjectRangeFilter (transforms_3d.py:1950-1992: strict in_range_bev on pcd_range[[0, 1, 3, 4]], then
    limit_yaw(offset=0.5, period=2 pi)) and ObjectNameFilter (:2047-2074: labels in range(num_classes)).
    boxes [G, 7 or 9] (x, y, z, dx, dy, dz, yaw[, vx, vy]), labels [G] int -> (float32 tensor [K, .], int array [K])."""
    t = torch.as_tensor(np.asarray(boxes), dtype=torch.float32).clone()
    labels = np.asarray(labels)
    angle, rot_mat_T = _box_rot_mat_T(t, aug["theta"])
    t[:, :3] = t[:, :3] @ rot_mat_T
    t[:, 6] += angle
    if t.shape[1] == 9:
        t[:, 7:9] = t[:, 7:9] @ rot_mat_T[:2, :2]
    t[:, :3] += t.new_tensor(np.asarray(aug["translation"]))
    t[:, :6] *= aug["scale"]
    t[:, 7:] *= aug["scale"]
    if aug.get("flip_horizontal"):
        t[:, 1::7] = -t[:, 1::7]
        t[:, 6] = -t[:, 6] + np.pi
    if aug.get("flip_vertical"):
        t[:, 0::7] = -t[:, 0::7]
        t[:, 6] = -t[:, 6]
    bev = np.array(point_cloud_range, dtype=np.float32)[[0, 1, 3, 4]]
    mask = (t[:, 0] > bev[0]) & (t[:, 1] > bev[1]) & (t[:, 0] < bev[2]) & (t[:, 1] < bev[3])
    t, labels = t[mask], labels[mask.numpy().astype(bool)]
    period = 2 * np.pi
    t[:, 6] = t[:, 6] - torch.floor(t[:, 6] / period + 0.5) * period
    keep = np.array([n in range(num_classes) for n in labels], dtype=np.bool_)
    return t[torch.from_numpy(keep)], labels[keep]


# ======================================================================================================================
# camera side: host tables of isf_image_prepass
PRECISION_BITS = 22      # Pillow's 8-bit resample path keeps coefficients with 22 fractional bits


@functools.lru_cache(maxsize=512)
def resample_tables(in_size, out_size):
    """Pillow's antialiased bicubic coefficients for one axis, in_size -> out_size, as the integers its 8-bit path
    multiplies with: (bounds int32 [out, 2] = (first input index, taps), coeffs int32 [out, ksize], zero past the taps).
    Float64 in Pillow's operation order; the weights of one output index are summed one after the other (adding the
    exact zeros past the taps changes nothing).  An axis that keeps its size is not resampled by Pillow: taps = 1 with
    coefficient 2^22 reproduces every byte."""
    if in_size == out_size:
        bounds = np.stack([np.arange(out_size), np.ones(out_size, np.int64)], 1)
        return bounds.astype(np.int32), np.full((out_size, 1), 1 << PRECISION_BITS, np.int32)
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0.0)
    xmax = np.minimum(np.trunc(center + support + 0.5), float(in_size)) - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    t = np.abs((x + xmin[:, None] - center[:, None] + 0.5) * ss)
    a = -0.5
    w = np.where(t < 1.0, ((a + 2.0) * t - (a + 3.0)) * t * t + 1,
                 np.where(t < 2.0, (((t - 5) * t + 8) * t - 4) * a, 0.0))
    w = np.where(x < xmax[:, None], w, 0.0)
    ww = np.zeros(out_size)
    for j in range(ksize):
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    one = float(1 << PRECISION_BITS)
    coeffs = np.where(w < 0, np.trunc(-0.5 + w * one), np.trunc(0.5 + w * one)).astype(np.int32)
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= in_size).all()
    assert (bounds[:, 1] <= ksize).all()
    return bounds, coeffs


def rotation_fixed(angle, width, height):
    """The six 16.16 integers of Pillow's Image.rotate(angle) (nearest, about (w / 2, h / 2), same size) or None when
    angle % 360 == 0 (Pillow returns a copy): output (x, y) reads ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16)."""
    angle = angle % 360.0
    if angle == 0:
        return None
    cx, cy = width / 2.0, height / 2.0
    t = -math.radians(angle)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    m[2] = m[0] * (-cx) + m[1] * (-cy) + m[2]
    m[5] = m[3] * (-cx) + m[4] * (-cy) + m[5]
    m[2] += cx
    m[5] += cy

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5),
            fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def normalize_table(mean, std):
    """ToTensor + Normalize of every byte value: float32 [3, 256], the float32 torch ops torchvision runs
    (uint8 -> float32, div(255), sub_(mean), div_(std))"""
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    mean, std = torch.as_tensor(mean, dtype=torch.float32), torch.as_tensor(std, dtype=torch.float32)
    return v[None, :].repeat(3, 1).sub_(mean[:, None]).div_(std[:, None]).numpy()


def image_aug_matrix(resize, crop, flip, rotate):
    """img_aug_matrix of one view: ImageAug3D.img_transform's post-homography (transforms_3d.py:92-110) in float32 torch
    ops in the reference's order, placed into eye(4) as __call__ does (:136-138)"""
    rotation, translation = torch.eye(2), torch.zeros(2)
    rotation *= float(resize)
    translation -= torch.Tensor(list(crop[:2]))
    if flip:
        A = torch.Tensor([[-1, 0], [0, 1]])
        b = torch.Tensor([crop[2] - crop[0], 0])
        rotation = A.matmul(rotation)
        translation = A.matmul(translation) + b
    theta = rotate / 180 * np.pi
    A = torch.Tensor([[np.cos(theta), np.sin(theta)], [-np.sin(theta), np.cos(theta)]])
    b = torch.Tensor([crop[2] - crop[0], crop[3] - crop[1]]) / 2
    b = A.matmul(-b) + b
    rotation = A.matmul(rotation)
    translation = A.matmul(translation) + b
    transform = torch.eye(4)
    transform[:2, :2] = rotation
    transform[:2, 3] = translation
    return transform.numpy()


def _find_transform(pipeline, name):
    for t in pipeline:
        if t.get("type") == name:
            return t
        if "transforms" in t:          # MultiScaleFlipAug3D of the test pipeline
            found = _find_transform(t["transforms"], name)
            if found is not None:
                return found
    return None


class MultiViewImageLoader:
    """Batch replacement for ImageAug3D -> ImageNormalize of configs/isfusion/isfusion_0075voxel.py:238-352: decoded
    uint8 images of every view of every sample in, `img [B, N, 3, fH, fW]` float32 on the device and `img_aug_matrix
    [B, N, 4, 4]` out, bit for bit what Pillow and torchvision give.  Constructor arguments carry the reference's names
    (ImageAug3D: final_dim, resize_lim, bot_pct_lim, rot_lim, rand_flip, is_train; ImageNormalize: mean, std)."""

    def __init__(self, final_dim, resize_lim, bot_pct_lim, rot_lim, rand_flip, is_train, mean, std, device="cuda"):
        self.final_dim = (int(final_dim[0]), int(final_dim[1]))
        self.resize_lim, self.bot_pct_lim, self.rot_lim = list(resize_lim), list(bot_pct_lim), list(rot_lim)
        self.rand_flip, self.is_train = bool(rand_flip), bool(is_train)
        self.mean, self.std = list(mean), list(std)
        self.device = torch.device(device)
        self._lut = normalize_table(self.mean, self.std)
        self._pinned_img = self._pinned_par = self._uploaded = None

    @classmethod
    def from_config(cls, config, train=False, device="cuda"):
        """config: path of the unmodified configs/isfusion/isfusion_0075voxel.py, its variable dict, or the
        (train_pipeline, test_pipeline) lists alone -> the loader of the chosen pipeline's ImageAug3D + ImageNormalize"""
        if isinstance(config, str):
            from . import registry
            config = registry.load_config(config)
        if isinstance(config, dict):
            pipeline = config["train_pipeline" if train else "test_pipeline"]
        else:
            pipeline = config[0 if train else 1]
        aug, norm = _find_transform(pipeline, "ImageAug3D"), _find_transform(pipeline, "ImageNormalize")
        if aug is None or norm is None:
            raise KeyError("the pipeline has no ImageAug3D / ImageNormalize entry")
        kw = {k: v for k, v in aug.items() if k != "type"}
        return cls(mean=norm["mean"], std=norm["std"], device=device, **kw)

    # ------------------------------------------------------------------------------------------------ host side
    def sample_augmentation(self, ori_shape):
        """One draw for one view, ori_shape = (W, H): ImageAug3D.sample_augmentation (transforms_3d.py:57-80), numpy RNG
        consumed in its order, sizes and crops in its own double-precision expressions
        -> (resize, resize_dims, crop, flip, rotate)"""
        W, H = ori_shape
        fH, fW = self.final_dim
        if self.is_train:
            resize = np.random.uniform(*self.resize_lim)
            resize_dims = (int(W * resize), int(H * resize))
            newW, newH = resize_dims
            crop_h = int((1 - np.random.uniform(*self.bot_pct_lim)) * newH) - fH
            crop_w = int(np.random.uniform(0, max(0, newW - fW)))
            crop = (crop_w, crop_h, crop_w + fW, crop_h + fH)
            flip = False
            if self.rand_flip and np.random.choice([0, 1]):
                flip = True
            rotate = np.random.uniform(*self.rot_lim)
        else:
            resize = np.mean(self.resize_lim)
            resize_dims = (int(W * resize), int(H * resize))
            newW, newH = resize_dims
            crop_h = int((1 - np.mean(self.bot_pct_lim)) * newH) - fH
            crop_w = int(max(0, newW - fW) / 2)
            crop = (crop_w, crop_h, crop_w + fW, crop_h + fH)
            flip = False
            rotate = 0
        return resize, resize_dims, crop, flip, rotate

    def describe(self, shapes, draws):
        """Host half of isf_image_prepass for views of shapes [(H, W)] under draws [(resize, resize_dims, crop, flip,
        rotate)] -> (list of _lib.ImageView with src_offset filled for back-to-back images, int32 table blob)"""
        fH, fW = self.final_dim
        views, blobs, where, at, offset = [], [], {}, 0, 0

        def tables(n_in, n_out):
            nonlocal at
            key = (n_in, n_out)
            if key not in where:
                bounds, coeffs = resample_tables(n_in, n_out)
                where[key] = (at, at + bounds.size, coeffs.shape[1])
                blobs.extend((bounds.reshape(-1), coeffs.reshape(-1)))
                at += bounds.size + coeffs.size
            return where[key]

        for (H, W), (_, resize_dims, crop, flip, rotate) in zip(shapes, draws):
            newW, newH = int(resize_dims[0]), int(resize_dims[1])
            if newW < 1 or newH < 1 or crop[2] - crop[0] != fW or crop[3] - crop[1] != fH:
                raise _lib.IsfError(f"image pre-pass: resize_dims {resize_dims} / crop {crop} do not fit final_dim")
            if H / newH > 20:
                raise _lib.IsfError(f"image pre-pass: shrinking {H} rows to {newH} is outside what the kernel holds")
            v = _lib.ImageView()
            v.src_offset, v.src_w, v.src_h, v.resize_w, v.resize_h = offset, W, H, newW, newH
            v.crop_x, v.crop_y, v.flip = int(crop[0]), int(crop[1]), int(bool(flip))
            rot = rotation_fixed(rotate, fW, fH)
            v.rotate = int(rot is not None)
            v.rot = (ctypes.c_int32 * 6)(*(rot or [0] * 6))
            v.h_bounds, v.h_coeffs, v.h_ksize = tables(W, newW)
            v.v_bounds, v.v_coeffs, v.v_ksize = tables(H, newH)
            views.append(v)
            offset += H * W * 3
        return views, np.concatenate(blobs).astype(np.int32)

    @staticmethod
    def _pin(buf, nbytes):
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()
        return buf

    def _paste_ops(self, paste, imgs, B, N, total):
        """Host half of isf_image_paste: the plans' rectangle operations as descriptors, their patches placed behind
        the images (from byte `total` on) -> (PasteView bytes, PasteOp bytes, patches [(offset, array)], new total,
        (max ops on a view, max box width, max box height), mixup) or None when no plan touches an image."""
        if len(paste) != B:
            raise _lib.IsfError(f"paste holds {len(paste)} plans for {B} samples")
        views, ops, patches, offset, mixups = [], [], [], 0, set()
        most = box_w = box_h = 0
        for b in range(B):
            plan = paste[b]
            per_view = [[] for _ in range(N)]
            where = {}
            for op in (plan.image_ops if plan is not None else []):
                if not 0 <= op["view"] < N:
                    raise _lib.IsfError(f"GT-paste operation on view {op['view']} of {N}")
                mixups.add(float(plan.mixup))
                d = _lib.PasteOp()
                (d.y0, d.y1), (d.x0, d.x1) = op["rows"], op["cols"]
                if op["kind"] == "patch":
                    k = op["object"]
                    if k not in where:
                        patch = plan.objects[k]["patch"]
                        where[k] = total
                        patches.append((total, patch))
                        total += patch.size
                    ph, pw = plan.objects[k]["patch"].shape[:2]
                    if d.y1 - d.y0 > ph or d.x1 - d.x0 > pw:
                        raise _lib.IsfError(f"GT-paste: a {d.y1 - d.y0} x {d.x1 - d.x0} rectangle reads past its "
                                            f"{ph} x {pw} patch")
                    d.kind, d.patch_offset, d.patch_pitch = _lib.PASTE_PATCH, where[k], pw
                    (d.mask_y0, d.mask_y1), (d.mask_x0, d.mask_x1) = op["mask_rows"], op["mask_cols"]
                else:
                    d.kind = _lib.PASTE_MIX
                per_view[op["view"]].append(d)
            for v in range(N):
                im, mine = imgs[b * N + v], per_view[v]
                H, W = im.shape[:2]
                pv = _lib.PasteView()
                pv.src_offset, pv.width, pv.height = offset, W, H
                pv.op_begin, pv.op_end = len(ops), len(ops) + len(mine)
                if mine:
                    if any(d.x0 < 0 or d.y0 < 0 or d.x1 > W or d.y1 > H or d.x0 >= d.x1 or d.y0 >= d.y1 for d in mine):
                        raise _lib.IsfError("GT-paste: an operation's rectangle leaves its view")
                    pv.box_x0, pv.box_y0 = min(d.x0 for d in mine), min(d.y0 for d in mine)
                    pv.box_x1, pv.box_y1 = max(d.x1 for d in mine), max(d.y1 for d in mine)
                    box_w, box_h = max(box_w, pv.box_x1 - pv.box_x0), max(box_h, pv.box_y1 - pv.box_y0)
                most = max(most, len(mine))
                ops.extend(mine)
                views.append(pv)
                offset += im.size
        if not ops:
            return None
        if len(mixups) != 1:
            raise _lib.IsfError(f"the plans of one batch share one mixup; got {sorted(mixups)}")
        if most > _lib.PASTE_MAX_OPS:
            raise _lib.IsfError(f"GT-paste: {most} operations on one view, at most {_lib.PASTE_MAX_OPS} are walked")
        return (b"".join(bytes(v) for v in views), b"".join(bytes(d) for d in ops), patches, total,
                (most, box_w, box_h), mixups.pop())

    def stage(self, results_list, aug=None, paste=None):
        """Host half of a call: draws, descriptors and tables, and the two uploads from pinned memory.  paste: None or
        per sample a gt_paste.GTPastePlan or None; the plans' patches are uploaded behind the images and their
        operations behind the tables.  -> dict for launch() (device buffers `raw` and `par`, the views' count and
        layout, `img_aug_matrix`)."""
        if self.device.type != "cuda":
            raise _lib.IsfError("MultiViewImageLoader runs on the GPU only (isf_image_prepass); no CPU fallback")
        B = len(results_list)
        imgs = [np.asarray(im) for res in results_list for im in res["img"]]
        N = len(results_list[0]["img"])
        if any(len(res["img"]) != N for res in results_list):
            raise _lib.IsfError("every sample of a batch needs the same number of views")
        for im in imgs:
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise _lib.IsfError(f"views are decoded uint8 [H, W, 3] images; got {im.dtype} {im.shape}")
        if aug is None:
            draws = [self.sample_augmentation((im.shape[1], im.shape[0])) for im in imgs]
        else:
            draws = [d for sample in aug for d in sample]
        views, tables = self.describe([im.shape[:2] for im in imgs], draws)
        matrices = torch.from_numpy(np.stack([image_aug_matrix(d[0], d[2], d[3], d[4]) for d in draws]))

        # the staging buffers are reused: the previous call's uploads (issued a whole call ago) must have left them
        if self._uploaded is not None:
            self._uploaded.synchronize()
        total = sum(im.size for im in imgs)
        pasted = None if paste is None else self._paste_ops(paste, imgs, B, N, total)
        if pasted is not None:
            total = pasted[3]
        self._pinned_img = self._pin(self._pinned_img, total)
        host = self._pinned_img.numpy()
        at = 0
        for im in imgs:
            host[at:at + im.size] = im.reshape(-1)
            at += im.size
        vbytes = np.frombuffer(b"".join(bytes(v) for v in views), dtype=np.uint8)
        params = np.concatenate([vbytes, tables.view(np.uint8), self._lut.reshape(-1).view(np.uint8)])
        extra = {}
        if pasted is not None:
            pv_bytes, op_bytes, patches, _, limits, mixup = pasted
            for where, patch in patches:
                host[where:where + patch.size] = patch.reshape(-1)
            pad = (-params.size) % 8                      # the descriptors hold 64-bit offsets
            extra = dict(paste=dict(views_at=params.size + pad, ops_at=params.size + pad + len(pv_bytes), limits=limits,
                                    mixup=mixup))
            params = np.concatenate([params, np.zeros(pad, np.uint8), np.frombuffer(pv_bytes, dtype=np.uint8),
                                     np.frombuffer(op_bytes, dtype=np.uint8)])
        self._pinned_par = self._pin(self._pinned_par, params.size)
        self._pinned_par.numpy()[:params.size] = params
        with torch.cuda.device(self.device):
            raw = self._pinned_img[:total].to(self.device, non_blocking=True)
            par = self._pinned_par[:params.size].to(self.device, non_blocking=True)
            if self._uploaded is None:
                self._uploaded = torch.cuda.Event()
            self._uploaded.record()
        return dict(raw=raw, par=par, tables_at=vbytes.size, lut_at=vbytes.size + tables.size * 4, batch=B, views=N,
                    img_aug_matrix=matrices.view(B, N, 4, 4), draws=draws, **extra)

    def paste(self, staged):
        """Device half of the GT-paste: one isf_image_paste launch, in place on staged['raw'] (a no-op for a batch whose
        plans touch no image).  launch() calls it; it is separate so that the pasted bytes can be looked at."""
        p = staged.pop("paste", None)
        if p is None:
            return
        base = staged["par"].data_ptr()
        mixup = float(p["mixup"])
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().isf_image_paste(
                _lib.ptr(staged["raw"]), base + p["views_at"], staged["batch"] * staged["views"], base + p["ops_at"],
                p["limits"][0], p["limits"][1], p["limits"][2], mixup, 1 - mixup, float(np.float32(mixup)),
                _lib.stream()), "isf_image_paste")

    def launch(self, staged, out=None):
        """Device half: one isf_image_prepass launch over staged buffers (after isf_image_paste when the batch carries
        GT-paste plans) -> img [B, N, 3, fH, fW] float32"""
        fH, fW = self.final_dim
        B, N = staged["batch"], staged["views"]
        self.paste(staged)
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty((B * N, 3, fH, fW), dtype=torch.float32, device=self.device)
            elif (out.dtype != torch.float32 or out.device.type != "cuda" or not out.is_contiguous()
                  or out.numel() != B * N * 3 * fH * fW):
                raise _lib.IsfError("image pre-pass: `out` must be a contiguous float32 device tensor of the output's size")
            base = staged["par"].data_ptr()
            _lib.check(_lib.load().isf_image_prepass(_lib.ptr(staged["raw"]), base, B * N, base + staged["tables_at"],
                                                     base + staged["lut_at"], fH, fW, _lib.ptr(out), _lib.stream()),
                       "isf_image_prepass")
        return out.view(B, N, 3, fH, fW)

    def __call__(self, results_list, aug=None, out=None, paste=None):
        """results_list: one dict per sample with 'img' = its views, each uint8 [H, W, 3] RGB (an array or anything
        np.asarray turns into one; sizes may differ per view).  aug: None (one sample_augmentation((W, H)) draw per view,
        in sample then view order) or per sample a list of (resize, resize_dims, crop, flip, rotate) per view.
        out: None or a contiguous float32 device tensor of B * N * 3 * fH * fW elements to write into.
        paste: None or per sample a gt_paste.GTPastePlan or None: the image side of ObjectSampleV2 (dbsampler.py:779-831)
        runs on the uploaded bytes before the pre-pass.
        -> (img [B, N, 3, fH, fW] float32 on the device, img_aug_matrix [B, N, 4, 4] float32).  Two uploads from pinned
        memory and one launch (two with plans); nothing is read back."""
        staged = self.stage(results_list, aug, paste)
        return self.launch(staged, out), staged["img_aug_matrix"]
