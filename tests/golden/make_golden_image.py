"""Generate tests/golden/image_ref.npz and tests/golden/isfusion_0075voxel_pipelines.txt with the REFERENCE's own code.

    python tests/golden/make_golden_image.py         # authoring container only (reference tree + Pillow)

Camera side: the reference's ImageAug3D and ImageNormalize (datasets/pipelines/transforms_3d.py:24-145), loaded through
ref_harness.install_pipelines(), run on PIL.Image.fromarray(...) inputs with the real Pillow installed here
(PIL 12.2.0 when the committed file was made; the version is stored in the file).  torchvision is absent and stubbed
EMPTY by the harness; ImageNormalize needs torchvision.transforms.{Compose, ToTensor, Normalize}, so three stand-ins
restate torchvision's documented definitions (ToTensor: HWC uint8 -> CHW float32 / 255; Normalize: (x - mean) / std
per channel, in place on a clone, float32).  Fixed draws go through the reference's __call__ too, with
sample_augmentation returning the chosen draw.

Box side: the reference's real LiDARInstance3DBoxes (core/bbox/structures/{utils, base_box3d, lidar_box3d}.py; only
mmdet3d.ops.iou3d.iou3d_cuda and mmdet3d.ops.roiaware_pool3d.points_in_boxes_gpu are stubbed, which these methods never
call) through GlobalRotScaleTransV2, RandomFlip3DV2, ObjectRangeFilter and ObjectNameFilter.  Two environment shims,
neither touching the reference's files: ObjectRangeFilter spells `np.bool` (:1985), which numpy 2 no longer has, so
`np.bool = bool` is set; and the box class names transforms_3d imported from the harness's inert stubs are pointed at
the real class (LiDAR) / empty classes (Depth, Camera) so that its isinstance checks work.

Inputs are NOT stored: tests regenerate them from tests/image_common.py.  Only numeric arrays are written."""
import ast
import os
import pprint
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import image_common as ic  # noqa: E402
import ref_harness  # noqa: E402


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class ToTensor:
    def __call__(self, pic):
        a = np.array(pic, np.uint8, copy=True)
        return torch.from_numpy(a).permute(2, 0, 1).contiguous().to(dtype=torch.float32).div(255)


class Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, tensor):
        tensor = tensor.clone()
        mean = torch.as_tensor(self.mean, dtype=tensor.dtype)
        std = torch.as_tensor(self.std, dtype=tensor.dtype)
        return tensor.sub_(mean[:, None, None]).div_(std[:, None, None])


def camera(t3d, out):
    import PIL
    from PIL import Image
    out["pil_version"] = np.array([int(v) for v in PIL.__version__.split(".")[:3]], np.int64)
    norm = t3d.ImageNormalize(mean=ic.MEAN, std=ic.STD)
    for name, case in ic.CASES.items():
        aug = t3d.ImageAug3D(final_dim=case["final_dim"], **case["loader"])
        drawn = []
        real = aug.sample_augmentation
        fixed = iter(case.get("draws", ()))

        def sample(data, real=real, fixed=fixed, drawn=drawn, name=name):
            d = next(fixed, None) if "draws" in ic.CASES[name] else None
            if d is None:
                d = real(data)
            drawn.append(d)
            return d

        aug.sample_augmentation = sample
        if "seed" in case:
            np.random.seed(case["seed"])
        elif name == "full":
            np.random.seed(ic.FULL_SEED)
        u8, f32, mats = [], [], []
        for sample_imgs in ic.case_images(name):
            h, w = sample_imgs[0].shape[:2]
            data = dict(img=[Image.fromarray(a) for a in sample_imgs], ori_shape=(w, h))
            if len({a.shape for a in sample_imgs}) > 1:       # mixed sizes: the reference reads one ori_shape per sample
                assert "draws" in case
            data = aug(data)
            u8 += [np.asarray(im).copy() for im in data["img"]]
            mats += [np.asarray(m) for m in data["img_aug_matrix"]]
            f32 += [t.numpy() for t in norm(dict(img=list(data["img"])))["img"]]
        u8 = np.stack(u8)
        out[name + "_draws"] = ic.pack_draws(drawn)
        out[name + "_aug_matrix"] = np.stack(mats).astype(np.float32)
        if name == "full":
            out["full_crc"] = np.array([ic.summarize(a)[0] for a in u8], np.uint32)
            out["full_sums"] = np.stack([ic.summarize(a)[1] for a in u8])
            out["full_samples"] = np.stack([a.reshape(-1)[ic.sample_positions(v, a.size)] for v, a in enumerate(u8)])
            out["full_f32_samples"] = np.stack([f32[v].reshape(-1)[ic.sample_positions(v, f32[v].size)]
                                                for v in range(len(f32))])
        else:
            out[name + "_u8"] = u8
            out[name + "_f32_view0"] = f32[0]
        print(name, u8.shape, "zero share", float((u8 == 0).mean()), "255 share", float((u8 == 255).mean()))


def boxes(t3d, out):
    ref_harness._mod("mmdet3d.ops.roiaware_pool3d", points_in_boxes_gpu=None)
    sys.modules["mmdet3d.ops.iou3d"].iou3d_cuda = None
    pkg = "mmdet3d.core.bbox.structures"
    sys.modules[pkg].__path__ = [os.path.join(ref_harness.REF, "mmdet3d", "core", "bbox", "structures")]
    for n in ("utils", "base_box3d", "lidar_box3d"):
        ref_harness._load(f"{pkg}.{n}", f"mmdet3d/core/bbox/structures/{n}.py")
    Boxes = sys.modules[pkg + ".lidar_box3d"].LiDARInstance3DBoxes
    t3d.LiDARInstance3DBoxes = Boxes
    t3d.DepthInstance3DBoxes = type("DepthInstance3DBoxes", (), {})
    t3d.CameraInstance3DBoxes = type("CameraInstance3DBoxes", (), {})
    if not hasattr(np, "bool"):
        np.bool = bool
    names = [f"class{i}" for i in range(ic.NUM_CLASSES)]
    for i, seed in enumerate(ic.BOX_SEEDS):
        limits = ic.box_limits(i)
        b, labels = ic.gt_boxes(seed)
        data = dict(gt_bboxes_3d=Boxes(b.copy(), box_dim=9), gt_labels_3d=labels.copy(), bbox3d_fields=["gt_bboxes_3d"])
        np.random.seed(seed)
        data = t3d.GlobalRotScaleTransV2(is_train=True, **limits)(data)
        data = t3d.RandomFlip3DV2()(data)
        data = t3d.ObjectRangeFilter(point_cloud_range=ic.PC_RANGE)(data)
        data = t3d.ObjectNameFilter(classes=names)(data)
        out[f"boxes{i}_lidar_aug_matrix"] = np.asarray(data["lidar_aug_matrix"], np.float32)
        out[f"boxes{i}_out"] = data["gt_bboxes_3d"].tensor.numpy()
        out[f"boxes{i}_labels"] = np.asarray(data["gt_labels_3d"], np.int64)
        print("boxes", i, "kept", len(out[f"boxes{i}_labels"]), "of", len(labels))


def pipelines():
    from isfusion_amd import registry
    cfg = registry.load_config(os.path.join(ref_harness.REF, "configs", "isfusion", "isfusion_0075voxel.py"))
    both = dict(train_pipeline=cfg["train_pipeline"], test_pipeline=cfg["test_pipeline"])
    text = pprint.pformat(both, width=120, sort_dicts=False) + "\n"
    assert ast.literal_eval(text) == both
    with open(os.path.join(HERE, "isfusion_0075voxel_pipelines.txt"), "w") as f:
        f.write(text)


def main():
    t3d = ref_harness.install_pipelines()["transforms_3d"]
    sys.modules["torchvision"].transforms = types.SimpleNamespace(Compose=Compose, ToTensor=ToTensor, Normalize=Normalize)
    out = {}
    camera(t3d, out)
    boxes(t3d, out)
    path = os.path.join(HERE, "image_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    pipelines()


if __name__ == "__main__":
    main()
