"""Time the camera input pre-pass (isf_image.hip, input_pipeline.MultiViewImageLoader) on one GPU with device events
after warm-up, at the sizes users run: B = 4 and B = 2 samples x 6 views, 1600 x 900 -> 384 x 1056, under the test-time
draw and under seeded training draws.  Per configuration, three repeats, alternating:
  * kernel     isf_image_prepass from device-resident uint8 to img (MultiViewImageLoader.launch)
  * loader     the whole call: draws' tables, staging into pinned memory, the two uploads, the launch
  * torch      the composition a user would otherwise write with stock torch on the same GPU, from the same
               device-resident uint8: F.interpolate(mode="bicubic", antialias=True) on the float image, slice-crop into
               zeros, flip, F.grid_sample(mode="nearest") for the rotation, normalise.  NOT bit-exact to Pillow: a
               yardstick for time only (views that share a draw run as one batch, the rest one by one).
and the algorithmic bytes (the source window the crop needs + the output) over the kernel time as a share of the
6.3 TB/s achievable HBM rate.

    python tools/image_bench.py [--steps 200] [--warmup 10] [--repeats 3]

Prints one JSON line per configuration."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_common as ic  # noqa: E402
from isfusion_amd import input_pipeline as ip  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
FINAL_DIM, SRC_HW = (384, 1056), (900, 1600)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def torch_prepass(views_u8, draws, mean, std):
    """stock-torch composition on the device; views_u8: list of uint8 [H, W, 3] device tensors"""
    fH, fW = FINAL_DIM
    groups = {}
    for i, d in enumerate(draws):
        groups.setdefault((d[1], d[2], d[3], float(d[4]), tuple(views_u8[i].shape)), []).append(i)
    out = torch.empty((len(draws), 3, fH, fW), dtype=torch.float32, device=views_u8[0].device)
    for (dims, crop, flip, rotate, _), idx in groups.items():
        x = torch.stack([views_u8[i] for i in idx]).permute(0, 3, 1, 2).float()
        x = F.interpolate(x, size=(dims[1], dims[0]), mode="bicubic", antialias=True, align_corners=False)
        y = x.new_zeros((len(idx), 3, fH, fW))
        l, t, r, b = crop
        sl, st, sr, sb = max(l, 0), max(t, 0), min(r, dims[0]), min(b, dims[1])
        y[:, :, st - t:sb - t, sl - l:sr - l] = x[:, :, st:sb, sl:sr]
        if flip:
            y = y.flip(-1)
        if rotate % 360.0 != 0:
            a = -math.radians(rotate)
            theta = torch.tensor([[math.cos(a), math.sin(a) * fH / fW, 0.0], [-math.sin(a) * fW / fH, math.cos(a), 0.0]],
                                 dtype=torch.float32, device=y.device)
            grid = F.affine_grid(theta[None].expand(len(idx), 2, 3), list(y.shape), align_corners=False)
            y = F.grid_sample(y, grid, mode="nearest", padding_mode="zeros", align_corners=False)
        out[idx] = (y / 255 - mean) / std
    return out


def window_bytes(views, tables):
    """source bytes the crops actually need, from the descriptors' own bounds tables"""
    fH, fW = FINAL_DIM
    total = 0
    for v in views:
        x0, x1 = max(v.crop_x, 0), min(v.crop_x + fW, v.resize_w) - 1
        y0, y1 = max(v.crop_y, 0), min(v.crop_y + fH, v.resize_h) - 1
        if x0 > x1 or y0 > y1:
            continue
        bh, bv = tables[v.h_bounds:].reshape(-1)[:2 * v.resize_w], tables[v.v_bounds:].reshape(-1)[:2 * v.resize_h]
        cols = bh[2 * x1] + bh[2 * x1 + 1] - bh[2 * x0]
        rows = bv[2 * y1] + bv[2 * y1 + 1] - bv[2 * y0]
        total += int(cols) * int(rows) * 3
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    base = [ic.image(500 + v, *SRC_HW) for v in range(6)]
    mean = torch.tensor(ic.MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(ic.STD, device=dev).view(1, 3, 1, 1)
    for batch in (4, 2):
        results = [dict(img=[np.roll(im, 37 * b, axis=1) for im in base]) for b in range(batch)]
        for mode, params in (("test", ic.TEST), ("train", ic.TRAIN)):
            loader = ip.MultiViewImageLoader(final_dim=FINAL_DIM, mean=ic.MEAN, std=ic.STD, device=dev, **params)
            np.random.seed(1234)
            draws = [[loader.sample_augmentation((SRC_HW[1], SRC_HW[0])) for _ in range(6)] for _ in range(batch)]
            flat = [d for s in draws for d in s]
            staged = loader.stage(results, draws)
            out = torch.empty((batch * 6, 3) + FINAL_DIM, dtype=torch.float32, device=dev)
            views_u8, at = [], 0
            for _ in flat:
                n = SRC_HW[0] * SRC_HW[1] * 3
                views_u8.append(staged["raw"][at:at + n].view(SRC_HW[0], SRC_HW[1], 3))
                at += n
            descs, tables = loader.describe([SRC_HW] * len(flat), flat)
            nbytes = window_bytes(descs, tables) + out.numel() * 4
            kernel, whole, stock = [], [], []
            for _ in range(a.repeats):
                kernel.append(timed(lambda: loader.launch(staged, out), a.steps, a.warmup))
                stock.append(timed(lambda: torch_prepass(views_u8, flat, mean, std), a.steps, a.warmup))
                whole.append(timed(lambda: loader(results, draws, out), a.steps, a.warmup))
            k = float(np.median(kernel))
            print(json.dumps(dict(
                what="image_prepass", batch=batch, views=batch * 6, draws=mode, steps=a.steps,
                kernel_ms=[round(x, 4) for x in kernel], loader_ms=[round(x, 3) for x in whole],
                torch_ms=[round(x, 3) for x in stock], algorithmic_mb=round(nbytes / 1e6, 1),
                hbm_share=round(nbytes / (k * 1e-3) / HBM_BYTES_PER_S, 3),
                torch_over_kernel=round(float(np.median(stock)) / k, 1))), flush=True)


if __name__ == "__main__":
    main()
