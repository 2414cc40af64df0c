"""CPU tests of the camera input pre-pass's host half and of the ground-truth side of the LiDAR augmentation
(isfusion_amd.input_pipeline) against tests/golden/image_ref.npz, which the reference's own ImageAug3D / ImageNormalize
(real Pillow), LiDARInstance3DBoxes, GlobalRotScaleTransV2, RandomFlip3DV2, ObjectRangeFilter and ObjectNameFilter made
(tests/golden/make_golden_image.py).  No GPU, no Pillow, no reference tree."""
import ast
import os

import numpy as np
import pytest
import torch

import image_common as ic
from isfusion_amd import _lib, input_pipeline as ip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "image_ref.npz"))


def _loader(name, device="cuda", **over):
    case = ic.CASES[name]
    return ip.MultiViewImageLoader(final_dim=case["final_dim"], mean=ic.MEAN, std=ic.STD, device=device,
                                   **dict(case["loader"], **over))


def _restate(name, ref):
    case = ic.CASES[name]
    draws = ic.unpack_draws(ref[name + "_draws"], case["final_dim"])
    imgs = [im for sample in ic.case_images(name) for im in sample]
    return [ic.prepass_u8(im, d, case["final_dim"], ip.resample_tables, ip.rotation_fixed) for im, d in zip(imgs, draws)]


# 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small_train", "small_fixed", "small_shrink"])
def test_host_tables_reproduce_pillow_small(ref, name):
    got = np.stack(_restate(name, ref))
    want = ref[name + "_u8"]
    assert got.shape == want.shape
    bad = int((got != want).sum())
    assert bad == 0, f"{bad} of {want.size} bytes differ from Pillow"


def test_host_tables_reproduce_pillow_full_size(ref):
    for v, got in enumerate(_restate("full", ref)):
        crc, sums = ic.summarize(got)
        assert np.array_equal(got.reshape(-1)[ic.sample_positions(v, got.size)], ref["full_samples"][v]), v
        assert np.array_equal(sums, ref["full_sums"][v]), v
        assert crc == int(ref["full_crc"][v]), v


def test_normalize_table_is_torchvision(ref):
    lut = ip.normalize_table(ic.MEAN, ic.STD)
    assert lut.dtype == np.float32 and lut.shape == (3, 256) and (np.diff(lut, axis=1) > 0).all()
    u8, f32 = ref["small_train_u8"][0], ref["small_train_f32_view0"]
    for c in range(3):
        assert np.array_equal(lut[c][u8[..., c]], f32[c])
    full = _restate("full", ref)
    for v, got in enumerate(full):
        chw = np.stack([lut[c][got[..., c]] for c in range(3)])
        assert np.array_equal(chw.reshape(-1)[ic.sample_positions(v, chw.size)], ref["full_f32_samples"][v])
    assert np.array_equal(ic.to_u8(np.stack([lut[c][full[0][..., c]] for c in range(3)]), lut), full[0])


def test_identity_table_and_bounds():
    b, k = ip.resample_tables(37, 37)
    assert np.array_equal(b[:, 0], np.arange(37)) and (b[:, 1] == 1).all() and (k == 1 << 22).all()
    for n_in, n_out in ((1600, 912), (900, 513), (200, 214), (112, 63), (900, 23)):
        b, k = ip.resample_tables(n_in, n_out)
        assert b.dtype == np.int32 and k.dtype == np.int32 and k.shape[0] == n_out
        assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] <= k.shape[1]).all()
        assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b.sum(1)) >= 0).all()      # windows move forward only
        assert np.abs(k).max() < 1 << 23       # negative lobes push a weight past one; a signed 24-bit operand holds it
        assert (np.abs(k.sum(1) - (1 << 22)) <= k.shape[1]).all()                    # weights sum to one


# 2 ------------------------------------------------------------------------------------------------------------------
def test_sample_augmentation_follows_the_reference_rng(ref):
    loader = _loader("small_train", device="cpu")
    np.random.seed(ic.CASES["small_train"]["seed"])
    draws = [loader.sample_augmentation((200, 112)) for _ in range(12)]
    assert np.array_equal(ic.pack_draws(draws), ref["small_train_draws"])
    np.random.seed(ic.FULL_SEED)
    assert np.array_equal(ic.pack_draws([_loader("full", device="cpu").sample_augmentation((1600, 900))]),
                          ref["full_draws"][3:])
    test_draw = _loader("full", device="cpu", **ic.TEST).sample_augmentation((1600, 900))
    assert np.array_equal(ic.pack_draws([test_draw]), ref["full_draws"][:1])
    assert test_draw[1] == (1152, 648) and test_draw[2] == (48, 264, 1104, 648)


@pytest.mark.parametrize("name", list(ic.CASES))
def test_img_aug_matrix_bit_equal(ref, name):
    draws = ic.unpack_draws(ref[name + "_draws"], ic.CASES[name]["final_dim"])
    got = np.stack([ip.image_aug_matrix(d[0], d[2], d[3], d[4]) for d in draws])
    assert got.dtype == np.float32 and np.array_equal(got, ref[name + "_aug_matrix"])


# 3 ------------------------------------------------------------------------------------------------------------------
def _box_draw(i):
    lim = ic.box_limits(i)
    np.random.seed(ic.BOX_SEEDS[i])
    return ip.draw_train_aug(resize_lim=lim["resize_lim"], rot_lim=lim["rot_lim"], trans_lim=lim["trans_lim"])


@pytest.mark.parametrize("i", range(len(ic.BOX_SEEDS)))
def test_lidar_aug_matrix_bit_equal(ref, i):
    got = ip.lidar_aug_matrix(_box_draw(i))
    assert got.dtype == np.float32 and np.array_equal(got, ref[f"boxes{i}_lidar_aug_matrix"])


@pytest.mark.parametrize("i", range(len(ic.BOX_SEEDS)))
def test_augment_gt_boxes(ref, i):
    """Kept set, labels and every column bit-equal, except the outputs of the two matrix products (xyz @ rot_mat_T,
    vel @ rot_mat_T[:2, :2]), where the BLAS may fuse differently from the authoring machine: there
    |diff| <= 2 * 3 * 2^-24 * sum |a_i| |b_i| per element, the standard bound of a three-term float32 dot product taken on
    both sides."""
    aug = _box_draw(i)
    boxes, labels = ic.gt_boxes(ic.BOX_SEEDS[i])
    got, got_labels = ip.augment_gt_boxes(boxes, labels, aug, ic.PC_RANGE, ic.NUM_CLASSES)
    want, want_labels = ref[f"boxes{i}_out"], ref[f"boxes{i}_labels"]
    assert np.array_equal(got_labels, want_labels)
    got = got.numpy()
    assert got.shape == want.shape and got.dtype == np.float32 and len(want) >= 25
    assert np.array_equal(got[:, 3:7], want[:, 3:7])             # sizes and yaw: no matrix product involved
    assert (np.abs(want[:, 6]) <= np.pi).all()
    # the rows that were kept, in order: recover them by the (exactly scaled) sizes
    src = torch.from_numpy(boxes)
    keep = [int(np.flatnonzero((np.float32(aug["scale"]) * boxes[:, 3:6] == w[3:6]).all(1))[0]) for w in want]
    assert keep == sorted(keep)
    rot = np.abs(ip._box_rot_mat_T(src, aug["theta"])[1].numpy().astype(np.float64))
    s = abs(float(aug["scale"]))
    eps = 2 * 3 * 2.0 ** -24
    bound_xyz = eps * (np.abs(boxes[keep, :3].astype(np.float64)) @ rot) * s
    bound_vel = eps * (np.abs(boxes[keep, 7:9].astype(np.float64)) @ rot[:2, :2]) * s
    assert (np.abs(got[:, :3].astype(np.float64) - want[:, :3]) <= bound_xyz).all()
    assert (np.abs(got[:, 7:9].astype(np.float64) - want[:, 7:9]) <= bound_vel).all()


def test_border_boxes_and_unknown_labels(ref):
    """the identity draw leaves the rows pinned at +-54 where they are: strictly inside stays, outside goes; label -1 goes"""
    i = len(ic.BOX_SEEDS) - 1
    aug = _box_draw(i)
    assert aug["scale"] == 1.0 and aug["theta"] == 0.0 and not np.any(aug["translation"])
    boxes, labels = ic.gt_boxes(ic.BOX_SEEDS[i])
    got, got_labels = ip.augment_gt_boxes(boxes, labels, aug, ic.PC_RANGE, ic.NUM_CLASSES)
    r = np.abs(got[:, :2].numpy())
    assert (r < 54).all() and np.isclose(r, 53.9).any() and np.isclose(r, 53.95).any() and (got_labels >= 0).all()
    assert (labels == -1).any() and len(got_labels) == len(ref[f"boxes{i}_labels"])


def test_draw_train_aug_keeps_its_draws():
    np.random.seed(3)
    a = ip.draw_train_aug()
    np.random.seed(3)
    scale, theta = np.random.uniform(0.9, 1.1), np.random.uniform(-0.78539816, 0.78539816)
    assert a["scale"] == scale and a["theta"] == theta
    assert np.array_equal(a["rot_mat_T"], ip.rotation_matrix_T(-theta))


# 4 ------------------------------------------------------------------------------------------------------------------
def test_from_config_reads_the_shipped_pipelines():
    with open(os.path.join(GOLDEN, "isfusion_0075voxel_pipelines.txt")) as f:
        cfg = ast.literal_eval(f.read())
    for config in (cfg, (cfg["train_pipeline"], cfg["test_pipeline"])):
        train = ip.MultiViewImageLoader.from_config(config, train=True, device="cpu")
        test = ip.MultiViewImageLoader.from_config(config, device="cpu")
        for ld in (train, test):
            assert ld.final_dim == (384, 1056) and ld.bot_pct_lim == [0.0, 0.0]
            assert ld.mean == [0.485, 0.456, 0.406] and ld.std == [0.229, 0.224, 0.225]
        assert train.resize_lim == [0.57, 0.825] and train.rot_lim == [-5.4, 5.4] and train.rand_flip and train.is_train
        assert test.resize_lim == [0.72, 0.72] and test.rot_lim == [0.0, 0.0] and not test.rand_flip and not test.is_train


def test_from_config_reads_a_config_file(tmp_path):
    with open(os.path.join(GOLDEN, "isfusion_0075voxel_pipelines.txt")) as f:
        text = f.read()
    path = tmp_path / "cfg.py"
    path.write_text("both = " + text + "train_pipeline = both['train_pipeline']\ntest_pipeline = both['test_pipeline']\n")
    assert ip.MultiViewImageLoader.from_config(str(path), train=True, device="cpu").resize_lim == [0.57, 0.825]


def test_loader_has_no_cpu_fallback():
    loader = _loader("small_train", device="cpu")
    with pytest.raises(_lib.IsfError):
        loader([dict(img=[ic.image(0, 112, 200)])])


def test_describe_fills_descriptors():
    loader = _loader("small_fixed", device="cpu")
    case = ic.CASES["small_fixed"]
    shapes = [(h, w) for sample in case["views"] for _, h, w in sample]
    views, tables = loader.describe(shapes, case["draws"])
    assert len(views) == 12 and tables.dtype == np.int32
    at = 0
    for v, (h, w), d in zip(views, shapes, case["draws"]):
        assert (v.src_offset, v.src_w, v.src_h) == (at, w, h) and (v.resize_w, v.resize_h) == d[1]
        assert (v.crop_x, v.crop_y, v.flip) == (d[2][0], d[2][1], int(d[3])) and v.rotate == int(d[4] % 360 != 0)
        b, k = ip.resample_tables(w, d[1][0])
        assert np.array_equal(tables[v.h_bounds:v.h_bounds + b.size], b.reshape(-1)) and v.h_ksize == k.shape[1]
        assert np.array_equal(tables[v.h_coeffs:v.h_coeffs + k.size], k.reshape(-1))
        b, k = ip.resample_tables(h, d[1][1])
        assert np.array_equal(tables[v.v_bounds:v.v_bounds + b.size], b.reshape(-1)) and v.v_ksize == k.shape[1]
        assert np.array_equal(tables[v.v_coeffs:v.v_coeffs + k.size], k.reshape(-1))
        at += h * w * 3
    with pytest.raises(_lib.IsfError):
        loader.describe([(112, 200)], [(0.5, (100, 56), (0, 8, 100, 56), False, 0)])     # crop is not final_dim
