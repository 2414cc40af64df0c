"""Shared by tests/golden/make_golden_image.py, tests/test_image_pipeline.py and tests/test_gpu_image.py: the seeded
input images, the cases of tests/golden/image_ref.npz, and a numpy restatement of the image pre-pass (Pillow's
resize -> crop -> flip -> rotate in integer arithmetic) that CONSUMES THE PRODUCT'S OWN HOST TABLES
(input_pipeline.resample_tables / rotation_fixed), so that the host half of isf_image_prepass is pinned without a GPU.
"""
import zlib

import numpy as np

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
TRAIN = dict(resize_lim=[0.57, 0.825], bot_pct_lim=[0.0, 0.0], rot_lim=[-5.4, 5.4], rand_flip=True, is_train=True)
TEST = dict(resize_lim=[0.72, 0.72], bot_pct_lim=[0.0, 0.0], rot_lim=[0.0, 0.0], rand_flip=False, is_train=False)
SMALL_DIM, FULL_DIM = (48, 132), (384, 1056)
SAMPLES = 4096


def image(seed, h, w):
    """uint8 [h, w, 3]: a smooth ramp averaged with noise, plus ~5 % pure 255 and ~5 % pure 0 pixels so that the
    bicubic overshoot hits both ends of the clip"""
    rng = np.random.RandomState(seed)
    smooth = (np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[..., None] + np.array([0, 80, 160])) % 256
    img = ((smooth + rng.randint(0, 256, (h, w, 3))) // 2).astype(np.uint8)
    img[rng.rand(h, w) < 0.05] = 255
    img[rng.rand(h, w) < 0.05] = 0
    return img


def fixed_draw(src_hw, final_dim, resize, crop_w, flip, rotate, resize_dims=None):
    """(resize, resize_dims, crop, flip, rotate) as ImageAug3D.sample_augmentation shapes it, for chosen values"""
    H, W = src_hw
    fH, fW = final_dim
    dims = (int(W * resize), int(H * resize)) if resize_dims is None else resize_dims
    crop_h = dims[1] - fH
    return resize, dims, (crop_w, crop_h, crop_w + fW, crop_h + fH), bool(flip), rotate


# name -> dict(final_dim, views = [[(seed, h, w) per view] per sample], seed (training draws under np.random.seed) or
# draws (per view, flat)).  Whole outputs are stored for the small cases, CRC / sums / samples for the full-size one.
_S = (112, 200)
_T = (90, 160)
CASES = {
    "small_train": dict(final_dim=SMALL_DIM, views=[[(100 + 6 * b + v, 112, 200) for v in range(6)] for b in range(2)],
                        seed=7, loader=TRAIN),
    "small_fixed": dict(
        final_dim=SMALL_DIM, loader=TRAIN,
        views=[[(200, *_S), (201, *_S), (202, *_S), (203, *_S), (204, *_T), (205, *_S)],
               [(206, *_S), (207, *_T), (208, *_S), (209, *_S), (210, *_S), (211, *_T)]],
        draws=[fixed_draw(_S, SMALL_DIM, 0.57, 0, True, -5.4),           # crop wider than the resized image, flip
               fixed_draw(_S, SMALL_DIM, 0.8, 20, False, 0),             # rotate = 0, no flip
               fixed_draw(_S, SMALL_DIM, 0.8, 20, True, 0.0),            # rotate = 0.0, flip
               fixed_draw(_S, SMALL_DIM, 1.07, 40, True, 1.0),           # upscale
               fixed_draw(_T, SMALL_DIM, 1.0, 10, False, 3.3),           # resize_dims = source size (no resample)
               fixed_draw(_S, SMALL_DIM, 0.825, 33, False, 5.4),
               fixed_draw(_S, SMALL_DIM, 0.57, 0, False, 360.0),         # rotate % 360 = 0
               fixed_draw(_T, SMALL_DIM, 0.9, 5, True, -4.9),            # second source size in the batch
               fixed_draw(_S, SMALL_DIM, 1.0, 0, False, 2.0, resize_dims=(200, 80)),    # vertical pass only
               fixed_draw(_S, SMALL_DIM, 1.0, 0, True, -2.0, resize_dims=(150, 112)),   # horizontal pass only
               fixed_draw(_S, SMALL_DIM, 0.61, 5, True, 180.0),
               fixed_draw(_T, SMALL_DIM, 1.3, 50, False, -90.0)]),
    # a shrink by four: more source rows under a tile than the kernel's LDS rows hold at once (its chunked path)
    "small_shrink": dict(
        final_dim=SMALL_DIM, loader=TRAIN, views=[[(220, 400, 640), (221, 400, 640)]],
        draws=[fixed_draw((400, 640), SMALL_DIM, 0.25, 10, False, 2.0),
               fixed_draw((400, 640), SMALL_DIM, 0.22, 3, True, 0)]),
    "full": dict(
        final_dim=FULL_DIM, loader=TRAIN, views=[[(300, 900, 1600), (301, 900, 1600), (302, 900, 1600), (303, 900, 1600)]],
        draws=[fixed_draw((900, 1600), FULL_DIM, 0.72, 48, False, 0),    # the test-time draw: crop (48, 264)
               fixed_draw((900, 1600), FULL_DIM, 0.57, 0, True, -5.4),
               fixed_draw((900, 1600), FULL_DIM, 0.825, 100, False, 5.4),
               None]),                                                   # one training draw under np.random.seed(11)
}
FULL_SEED = 11


def case_images(name):
    return [[image(*v) for v in sample] for sample in CASES[name]["views"]]


def pack_draws(draws):
    """float64 [V, 7]: resize, resize_w, resize_h, crop_x, crop_y, flip, rotate (the crop is final_dim wide and high)"""
    return np.array([[d[0], d[1][0], d[1][1], d[2][0], d[2][1], float(d[3]), d[4]] for d in draws], np.float64)


def unpack_draws(arr, final_dim):
    fH, fW = final_dim
    return [(r[0], (int(r[1]), int(r[2])), (int(r[3]), int(r[4]), int(r[3]) + fW, int(r[4]) + fH), bool(r[5]), r[6])
            for r in arr]


def sample_positions(view, numel):
    return np.random.RandomState(9000 + view).randint(0, numel, size=SAMPLES)


def summarize(u8):
    """(crc32 of the bytes, per-channel sums) of one uint8 [fH, fW, 3] result"""
    return zlib.crc32(np.ascontiguousarray(u8).tobytes()), u8.reshape(-1, 3).sum(0).astype(np.int64)


# ------------------------------------------------------------------------------------------------------ restatement
def _resample_axis1(img, out_size, tables):
    """one pass along axis 1 of uint8 [H, W, C] with the product's tables"""
    bounds, coeffs = tables(img.shape[1], out_size)
    out = np.zeros((img.shape[0], out_size, img.shape[2]), np.uint8)
    src = img.astype(np.int64)
    for xx in range(out_size):
        x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = (src[:, x0:x0 + n, :] * coeffs[xx, :n].astype(np.int64)[None, :, None]).sum(1) + (1 << 21)
        assert np.abs(acc).max() < 2 ** 31          # Pillow (and the kernel) accumulate in int32
        out[:, xx, :] = np.clip(acc >> 22, 0, 255)
    return out


def prepass_u8(img, draw, final_dim, tables, rotation_fixed):
    """resize (horizontal pass rounded to uint8, then vertical) -> crop with zero fill -> flip -> nearest rotation of one
    uint8 [H, W, 3] image -> uint8 [fH, fW, 3]"""
    _, (newW, newH), crop, flip, rotate = draw
    fH, fW = final_dim
    x = _resample_axis1(img, newW, tables)
    x = _resample_axis1(x.transpose(1, 0, 2), newH, tables).transpose(1, 0, 2)
    out = np.zeros((fH, fW, 3), np.uint8)
    l, t, r, b = crop
    sl, st, sr, sb = max(l, 0), max(t, 0), min(r, newW), min(b, newH)
    if sr > sl and sb > st:
        out[st - t:sb - t, sl - l:sr - l] = x[st:sb, sl:sr]
    if flip:
        out = out[:, ::-1]
    rot = rotation_fixed(rotate, fW, fH)
    if rot is None:
        return np.ascontiguousarray(out)
    a0, a1, a2, a3, a4, a5 = rot
    ys, xs = np.mgrid[0:fH, 0:fW].astype(np.int64)
    xin, yin = (a2 + ys * a1 + xs * a0) >> 16, (a5 + ys * a4 + xs * a3) >> 16
    ok = (xin >= 0) & (xin < fW) & (yin >= 0) & (yin < fH)
    res = np.zeros_like(out)
    res[ok] = out[yin[ok], xin[ok]]
    return res


def to_u8(img_f32, lut):
    """float32 [3, fH, fW] output of the pre-pass -> uint8 [fH, fW, 3] by EXACT membership in the (strictly increasing)
    normalise table; raises on any value that is not an entry"""
    out = np.empty(img_f32.shape[1:] + (3,), np.uint8)
    for c in range(3):
        assert (np.diff(lut[c]) > 0).all()
        idx = np.searchsorted(lut[c], img_f32[c])
        idx = np.minimum(idx, 255)
        if not np.array_equal(lut[c][idx], img_f32[c]):       # NaN fails here too
            raise AssertionError(f"channel {c}: {int((lut[c][idx] != img_f32[c]).sum())} values are not table entries")
        out[..., c] = idx
    return out


# ------------------------------------------------------------------------------------------------------ box fixtures
PC_RANGE = [-54, -54, -5, 54, 54, 3]
NUM_CLASSES = 10
BOX_SEEDS = (21, 22, 23, 24, 25)


def box_limits(i):
    """GlobalRotScaleTransV2 limits of draw i: the shipped training ones, and for the last draw the identity (scale 1,
    theta 0, no translation), under which the rows pinned at the border of the BEV range stay there"""
    if i == len(BOX_SEEDS) - 1:
        return dict(resize_lim=[1.0, 1.0], rot_lim=[0.0, 0.0], trans_lim=0.0)
    return dict(resize_lim=[0.9, 1.1], rot_lim=[-0.78539816, 0.78539816], trans_lim=0.5)


def gt_boxes(seed, count=48):
    """float32 [count, 9] boxes and int64 labels: centres up to and beyond the BEV range, rows pinned just inside /
    outside its border, labels in -1 .. 9, yaws that wrap past +-pi after rotation and flip"""
    rng = np.random.RandomState(seed)
    b = np.zeros((count, 9), np.float32)
    b[:, :2] = rng.uniform(-60, 60, (count, 2))
    b[:, 2] = rng.uniform(-3, 1, count)
    b[:, 3:6] = rng.uniform(0.5, 6, (count, 3))
    b[:, 6] = rng.uniform(-2 * np.pi, 2 * np.pi, count)
    b[:, 7:9] = rng.normal(0, 3, (count, 2))
    b[:4, :2] = [[53.9, 0], [54.1, 0], [0, -53.95], [0, -54.05]]
    b[4:8, 6] = [np.pi, -np.pi, 3.1, -3.1]
    labels = rng.randint(-1, NUM_CLASSES, count).astype(np.int64)
    labels[:4] = [3, 3, 5, 5]          # the border rows survive or fall by the range filter alone
    labels[8] = -1
    return b, labels
