"""tools/launch_balance_census.py -- CPU census behind the equal-work XCD parts: steps per XCD part
of the narrow launches of several rounds on the benchmark geometry, with the plain plan's equal-ROW parts and with the part
table's equal-WORK cuts (the arithmetic of csrc/isf_spconv16.h restated in numpy).

    python tools/launch_balance_census.py [--batch 4] [--points 300000] [--frame-set 0]

No GPU.  Steps of a 128-row tile = popcount of the OR of its rows' 27-bit tap masks x 32-channel chunks; the geometry is the
benchmark's frame set voxelized as the LiDAR branch does (0.075 m x 0.075 m x 0.2 m) and strided down once for level 1."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIXED = {32: 8, 64: 26}      # conv16_tile_fixed_steps of 32 -> 32 / 64 -> 64
TM = 128


def key(a, shape):
    return ((a[:, 0] * shape[0] + a[:, 1]) * shape[1] + a[:, 2]) * shape[2] + a[:, 3]


def down(c, shape, ks=(3, 3, 3), st=(2, 2, 2), pd=(1, 1, 1)):
    """output cells of a strided sparse conv over the cells c [n, 4] (b, z, y, x), sorted"""
    oshape = [(shape[d] + 2 * pd[d] - ks[d]) // st[d] + 1 for d in range(3)]
    outs = []
    for kz in range(ks[0]):
        for ky in range(ks[1]):
            for kx in range(ks[2]):
                k = (kz, ky, kx)
                o = np.empty_like(c)
                o[:, 0] = c[:, 0]
                ok = np.ones(len(c), bool)
                for d in range(3):
                    num = c[:, d + 1] + pd[d] - k[d]
                    od = num // st[d]
                    ok &= (num % st[d] == 0) & (od >= 0) & (od < oshape[d])
                    o[:, d + 1] = od
                outs.append(o[ok])
    return np.unique(np.concatenate(outs), axis=0), oshape


def submasks(c, shape):
    """27-bit tap masks of a SubM 3 x 3 x 3 conv over the sorted cells c"""
    ks = key(c, shape)
    m = np.zeros(len(c), np.uint32)
    t = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                n = c.copy()
                n[:, 1] += dz
                n[:, 2] += dy
                n[:, 3] += dx
                ok = ((n[:, 1:] >= 0) & (n[:, 1:] < np.array(shape))).all(1)
                kk = key(n, shape)
                pos = np.minimum(np.searchsorted(ks, kk), len(ks) - 1)
                m |= (ok & (ks[pos] == kk)).astype(np.uint32) << t
                t += 1
    return m


def tile_steps(masks, chunks, parts=8):
    """steps of every uniform tile of conv16_plan (parts x full tiles, tile t = tile t % full of part t // full)"""
    n = len(masks)
    part_rows = -(-(-(-n // 16)) // parts) * 16
    full = -(-part_rows // TM)
    w = np.zeros(parts * full, np.int64)
    for p in range(parts):
        for j in range(full):
            r0, r1 = p * part_rows + j * TM, min(p * part_rows + min((j + 1) * TM, part_rows), n)
            if r0 < r1:
                w[p * full + j] = bin(int(np.bitwise_or.reduce(masks[r0:r1]))).count("1") * chunks
    return w, full


def part_firsts(weights, parts, cap):
    """conv16_part_cut + conv16_part_firsts"""
    W, T = np.cumsum(weights), len(weights)
    first = [0]
    for k in range(1, parts):
        c = int(np.nonzero(W * parts >= k * W[-1])[0][0]) + 1
        first.append(max(min(max(c, first[-1]), first[-1] + cap), T - (parts - k) * cap))
    return first + [T]


def report(name, masks, chunks):
    steps, full = tile_steps(masks, chunks)
    T, live = len(steps), steps > 0
    even = [k * full for k in range(9)]
    cap = full + (full + 7) // 8 + 1
    first = part_firsts(np.where(live, steps + FIXED[32 * chunks], 0), 8, cap)
    print(f"== {name}: {len(masks)} rows, {int(live.sum())} tiles of {TM} rows, steps per tile min {steps[live].min()} "
          f"mean {steps[live].mean():.1f} max {steps.max()}; cap {cap} tiles per part")
    for label, cuts in (("equal rows", even), ("equal work", first)):
        s = np.array([steps[a:b].sum() for a, b in zip(cuts, cuts[1:])])
        t = np.array([int(live[a:b].sum()) for a, b in zip(cuts, cuts[1:])])
        print(f"   {label}: steps per part {s.tolist()}  heaviest {s.max() / s.mean():.3f} x mean; tiles per part {t.tolist()} "
              f"({t.min() / t.mean():.3f} .. {t.max() / t.mean():.3f} x the even share)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--frame-set", type=int, default=0)
    args = ap.parse_args()
    import bench
    rg, vs = np.array([-54.0, -54.0, -5.0]), np.array([0.075, 0.075, 0.2])
    cs = []
    for b, p in enumerate(bench.make_frames(0, 1, args.batch, args.points, args.frame_set)):
        c = np.floor((np.asarray(p)[:, :3].astype(np.float32) - rg.astype(np.float32)) / vs.astype(np.float32)).astype(np.int64)
        c = c[((c >= 0) & (c < np.array([1440, 1440, 40]))).all(1)][:, ::-1]
        cs.append(np.concatenate([np.full((len(c), 1), b), c], 1))
    shape0 = [41, 1440, 1440]
    c0 = np.unique(np.concatenate(cs), axis=0)
    c1, shape1 = down(c0, shape0)
    report("level 0, 32 -> 32", submasks(c0, shape0), 1)
    report("level 1, 64 -> 64", submasks(c1, shape1), 2)


if __name__ == "__main__":
    main()
