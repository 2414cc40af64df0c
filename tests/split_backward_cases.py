"""Inputs of the backward split-precision tier, shared by the GPU tests (tests/test_gpu_split_backward.py) and by the CPU
tests that show their bounds are left by each defect (tests/test_split_model.py).  numpy only."""
import numpy as np

import split_model as sm

# (cin, cout): one per distinct (BM, BN, WM, WN) of wgrad16_shape -- (32,32,1,1) (64,32,1,1) (32,64,1,1) (64,64,1,1)
# (64,64,2,2) twice (one / two workgroup columns) and (256,256)
CONV_SHAPES = [(32, 32), (64, 32), (32, 64), (64, 64), (128, 128), (128, 256), (256, 256)]
GRID = (9, 24, 20)
SUBM = (True, [3, 3, 3], [1, 1, 1], [1, 1, 1])
STRIDED = (False, [3, 3, 3], [2, 2, 2], [1, 1, 1])
# (gradient class, activation class) of the dW checks: every gradient class, every activation class A-E
PAIRS = [("Guni", "C"), ("Guni", "A"), ("Grow", "B"), ("Grow", "E_row"), ("Gspike", "D"), ("Gelem", "E_elem"),
         ("Gedge", "C")]
HALF_PAIRS = [("Guni", "C"), ("Grow", "E_row")]          # single-pass f16 (hi halves only), dX and dW
FACTORS = (2.0 ** -40, 2.0 ** 30)                        # scale equivariance (classes Guni and Grow)
LINEAR_SHAPES = [(700, 256, 256), (1000, 128, 384)]      # (M, K, N) of the dX GEMM: gradient [M, K], dX [M, N]
ROWS_WGRAD_SHAPES = [(64, 96), (256, 1024)]              # (N, K) next to R = 130 / the smallest chunked R; R = 1000


def conv_rows(cin, cout):
    """1000 rows (four pair chunks of 256 on the centre tap), 700 (three) from 128 x 128 channels on"""
    return 1000 if cin * cout <= 64 * 64 else 700


def geometry(seed, rows, grid=GRID, B=2):
    """`rows` seeded active cells (b, z, y, x) on the EVEN z planes of B grids, sorted: a SubM 3x3x3 rulebook then has no
    pair on its 18 taps with dz != 0, every row on the centre tap and ~rows^2 / cells on the other eight; a stride-2
    rulebook (padding 1) pairs nothing on the taps kz = 0 and 2"""
    rng = np.random.default_rng([seed, 5])
    D, H, W = grid
    zs = np.arange(0, D, 2)
    lin = np.sort(rng.choice(B * zs.size * H * W, rows, replace=False))
    return np.stack([lin // (zs.size * H * W), zs[(lin // (H * W)) % zs.size], (lin // W) % H, lin % W], 1).astype(np.int32)


def cpu_nbr(idx, grid, geo):
    """output-stationary neighbour table of a rulebook in numpy -> (nbr int64 [K, num_out], num_out): tap k = (kz, ky, kx)
    of output cell o reads input cell o * stride + k - padding.  SubM: the outputs are the inputs; else every cell some
    input reaches, sorted.  (The GPU tests take the table the library built; this one serves the CPU tests.)"""
    subm, ks, st, pd = geo
    idx = np.asarray(idx, dtype=np.int64)
    ks, st, pd, grid = (np.asarray(v, dtype=np.int64) for v in (ks, st, pd, grid))
    oshape = grid if subm else (grid + 2 * pd - ks) // st + 1
    taps = np.stack(np.unravel_index(np.arange(int(np.prod(ks))), ks), 1)
    lin = lambda c, shape: ((c[:, 0] * shape[0] + c[:, 1]) * shape[1] + c[:, 2]) * shape[2] + c[:, 3]
    if subm:
        out = idx
    else:
        cand = []
        for k in taps:
            num = idx[:, 1:] + pd - k
            ok = (num % st == 0).all(1) & (num // st >= 0).all(1) & (num // st < oshape).all(1)
            cand.append(np.concatenate([idx[ok, :1], num[ok] // st], 1))
        cand = np.concatenate(cand)
        out = cand[np.unique(lin(cand, oshape), return_index=True)[1]]
    key = lin(idx, grid)
    order = np.argsort(key)
    nbr = np.full((len(taps), len(out)), -1, np.int64)
    for t, k in enumerate(taps):
        src = out[:, 1:] * st + k - pd
        ok = (src >= 0).all(1) & (src < grid).all(1)
        want = lin(np.concatenate([out[:, :1], src], 1)[ok], grid)
        pos = np.minimum(np.searchsorted(key[order], want), len(key) - 1)
        hit = key[order][pos] == want
        nbr[t, np.flatnonzero(ok)[hit]] = order[pos[hit]]
    return nbr, len(out)


def dense_nbr(H, W):
    """the 3 x 3, padding 1 rulebook of one dense H x W map (token = y W + x), taps (ky, kx)"""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    idx = np.stack([0 * yy.ravel(), 0 * yy.ravel(), yy.ravel(), xx.ravel()], 1)
    return cpu_nbr(idx, (1, H, W), (True, [1, 3, 3], [1, 1, 1], [0, 1, 1]))[0]


def check_rulebook(nbr, wk, chunks3):
    """the properties a rulebook must have before a dW kernel whose waves own wp = 256 / wk pairs of a 256-pair chunk is
    judged on it -> pair counts.  (i) a tap without pairs; (ii) chunks3: a tap with three pair chunks or more.  Only a
    SubM rulebook can have one at 700 .. 1000 rows (its centre tap pairs every row): a stride-2 rulebook pairs a quarter
    of these rows per tap at most, one chunk, so there the demand is a tap longer than the 64 pairs of the narrowest
    wave range; (iii) five taps or more whose counts are no multiple of 32 and none of wp."""
    counts = (np.asarray(nbr) >= 0).sum(1)
    wp = 256 // wk
    assert (counts == 0).any() and (counts > 0).sum() >= 9
    assert counts.max() > (2 * 256 if chunks3 else 64)
    assert ((counts % 32 != 0) & (counts % wp != 0) & (counts > 0)).sum() >= 5
    return counts


def conv_weight(K, cin, cout, seed):
    return np.random.default_rng([seed, 21]).normal(0, (1.0 / (6 * cin)) ** 0.5, (K, cin, cout)).astype(np.float32)


def linear_weight(K, N, seed):
    return np.random.default_rng([seed, 41]).normal(0, (1.0 / (6 * K)) ** 0.5, (N, K)).astype(np.float32)


def poisoned_grad(shape, seed):
    """class Guni with GRAD_POISON planted: the infinity in row 0, the NaN and the finite 3.2e38 in two seeded rows
    -> (g, the three rows); the scale is still 1 (none of the three sets it)"""
    rng = np.random.default_rng([seed, 83])
    g = sm.make_grad("Guni", shape, seed)
    rows = np.concatenate([[0], 1 + rng.choice(shape[0] - 1, 2, replace=False)])
    for r, v in zip(rows, sm.GRAD_POISON):
        g[r, rng.integers(0, shape[1])] = v
    assert sm.grad_scale(g) == 1.0
    return g, rows


def factor(g, f):
    """g times the power of two f, exactly (asserted: nothing under- or overflows)"""
    out = (g.astype(np.float64) * f).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), g.astype(np.float64) * f)
    return out
