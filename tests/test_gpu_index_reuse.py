"""The level-0 occupancy index lives in persistent per-workspace arrays and a call writes only the words that are, or
were, non-zero (ByteMaps::bits0 / prefix0 / dirty, isf_runtime.hip).  What can go wrong is STATE: a word, a prefix or a dirty
byte left by an earlier call on the same stream.  Every test here runs several calls on one stream and asks that a result
does not depend on what ran before it: bit-equal to the same call made first on a freshly released workspace, and equal
to the CPU oracle.  Also here: the two forms of the index scan (block totals added by every block itself up to 8192 scan
blocks, which also sends the voxel count to the host; the single-workgroup scan above), and the rows of voxels cut by
64-record boundaries, which the mean kernel zeroes."""

import numpy as np
import pytest
import torch

from isfusion_amd import _lib

pytestmark = pytest.mark.gpu

VS = [0.075, 0.075, 0.2]
RG = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
GRID = (40, 1440, 1440)      # (z, y, x) cells of the 0.075 m grid
D_BRANCH = 41                # the LiDAR branch's index has the sparse encoder's depth, the stand-alone VFE's has GRID[0]
WORDS_PER_SCAN_BLOCK = 1024


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def fresh_workspace():
    """free every workspace of the library (persistent maps included): the next call starts from nothing"""
    torch.cuda.synchronize()
    _lib.check(_lib.load().isf_release_workspace(), "isf_release_workspace")


def cell_points(cells, rng, vs=VS, per_cell=2):
    """points inside the given (z, y, x) cells, `per_cell` each, well away from the cell faces; 5 columns"""
    c = np.repeat(np.asarray(cells, np.float64).reshape(-1, 3), per_cell, 0)
    lo = np.array([RG[0], RG[1], RG[2]]) + c[:, ::-1] * np.array(vs)
    xyz = lo + rng.uniform(0.25, 0.75, (len(c), 3)) * np.array(vs)
    return np.concatenate([xyz, rng.random((len(c), 2))], 1).astype(np.float32)


def word_cells(word, depth, frame, bits=(0, 1, 31, 62, 63), grid=GRID):
    """(z, y, x) of some cells of bitmap word `word` of an index [B, depth, y, x] that lie in frame `frame`"""
    out = []
    for b in bits:
        cell = word * 64 + b
        x = cell % grid[2]
        y = cell // grid[2] % grid[1]
        z = cell // (grid[2] * grid[1]) % depth
        assert cell // (grid[2] * grid[1] * depth) == frame and z < grid[0], (word, b)
        out.append((z, y, x))
    return out


def random_points(seed, n, spread=20.0):
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([rng.uniform(-spread, spread, (n, 2)), rng.uniform(-4.5, 2.5, (n, 1))], 1)
    return np.concatenate([xyz, rng.random((n, 2))], 1).astype(np.float32)


def coors_of(oracle_mod, frames, vs=VS):
    return np.concatenate([np.concatenate([np.full((len(p), 1), b, np.int32), oracle_mod.dynamic_voxelize(p, vs, RG)], 1)
                           for b, p in enumerate(frames)])


def oracle_vfe(oracle_mod, lb, frames, vs=VS):
    """(voxel features, voxel coordinates) of the CPU oracle for the branch's VFE weights (the module still on the CPU)"""
    from isfusion_amd.norm import fold_bn
    vfe = lb.pts_voxel_encoder
    bn1 = [t.numpy() for t in fold_bn(vfe.vfe_layers[0].norm)]
    bn2 = [t.numpy() for t in fold_bn(vfe.vfe_layers[1].norm)]
    coors = coors_of(oracle_mod, frames, vs)
    ovf, ovc, _ = oracle_mod.dynamic_vfe(np.concatenate(frames), coors, vs, RG,
                                         vfe.vfe_layers[0].linear.weight.detach().numpy(), bn1,
                                         vfe.vfe_layers[1].linear.weight.detach().numpy(), bn2)
    return coors, ovf, ovc


def make_branch(seed=0, voxel=None, side=None):
    import isfusion_amd as m
    from isfusion_amd.lidar_branch import ISFUSION_0075
    kw = {}
    if voxel is not None:
        kw = dict(voxel_size=[voxel, voxel, 0.2],
                  pts_middle_encoder=dict(ISFUSION_0075["pts_middle_encoder"], sparse_shape=[41, side, side]))
    return m.LidarBranch(**kw).randomize_weights_(seed).randomize_bn_(seed + 1).eval()


def frame_sets():
    """X: two ordinary frames.  Y: fewer, different voxels -- the first word, both sides of a scan-block boundary (words
    1023 | 1024), and in frame 1 the last word a point can reach and both sides of a block boundary there.  Z: a frame with
    points in the first word only and a frame with points in the last reachable word only."""
    rng = np.random.default_rng(11)
    frame_words = D_BRANCH * GRID[1] * GRID[2] // 64                    # 1 328 400: frame 1 starts inside a scan block
    last1 = (1 * D_BRANCH + GRID[0]) * GRID[1] * GRID[2] // 64 - 1      # last word of frame 1 below the padding plane z = 40
    edge1 = (frame_words // WORDS_PER_SCAN_BLOCK + 1) * WORDS_PER_SCAN_BLOCK   # first block boundary inside frame 1
    X = [random_points(1, 5000), random_points(2, 4000)]
    Y = [np.concatenate([cell_points(word_cells(0, D_BRANCH, 0) + word_cells(1023, D_BRANCH, 0) +
                                     word_cells(1024, D_BRANCH, 0), rng), random_points(3, 150, 6.0)]),
         np.concatenate([cell_points(word_cells(last1, D_BRANCH, 1) + word_cells(edge1 - 1, D_BRANCH, 1) +
                                     word_cells(edge1, D_BRANCH, 1), rng), random_points(4, 100, 6.0)])]
    Z = [cell_points(word_cells(0, D_BRANCH, 0), rng), cell_points(word_cells(last1, D_BRANCH, 1), rng)]
    return dict(X=X, Y=Y, Z=Z)


def test_lidar_branch_does_not_depend_on_the_calls_before_it(dev, oracle_mod):
    """X, Y, Z, X on one stream, the stand-alone VFE (another depth, so other words for the same cells) in between: every
    BEV map bit-equal to that frame set run first on a freshly released workspace; voxel coordinates equal to the oracle's,
    voxel features within the VFE tolerance of tests/test_gpu_parity.py (1e-4: fp32, another summation order)."""
    sets = frame_sets()
    lb = make_branch(0)
    want = {k: oracle_vfe(oracle_mod, lb, v) for k, v in sets.items()}
    assert len(want["Y"][2]) < len(want["X"][2]) and len(want["Z"][2]) == 10
    lb = lb.to(dev)
    first = {}
    for k, frames in sets.items():
        fresh_workspace()
        first[k] = lb([T(p, dev) for p in frames], want_stats=True).clone()
        assert lb.last_stats.num_in[0] == len(want[k][2]), k
        assert (first[k] != 0).any()
    fresh_workspace()
    for step, k in enumerate("XYZXZYX"):
        frames = sets[k]
        out = lb([T(p, dev) for p in frames], want_stats=True)
        assert lb.last_stats.num_in[0] == len(want[k][2]), (step, k)
        assert torch.equal(out, first[k]), (step, k)
        coors, ovf, ovc = want[k]
        vf, vc = lb.pts_voxel_encoder(T(np.concatenate(frames), dev), T(coors, dev))
        assert np.array_equal(vc.cpu().numpy(), ovc), (step, k)
        err = np.abs(vf.cpu().numpy() - ovf).max()
        assert err < 1e-4, (step, k, err)


def test_grid_change_on_one_workspace(dev, oracle_mod):
    """0.075 m voxels, then 0.15 m (a quarter of the words: the rest of the persistent arrays keeps the first call's
    words and dirty bytes), then 0.075 m again: the last map bit-equal to the first, the middle one to a fresh workspace's"""
    frames = [random_points(21, 3000), random_points(22, 2000)]
    fine, coarse = make_branch(0), make_branch(2, voxel=0.15, side=720)
    _, _, ovc_f = oracle_vfe(oracle_mod, fine, frames)
    _, _, ovc_c = oracle_vfe(oracle_mod, coarse, frames, [0.15, 0.15, 0.2])
    fine, coarse = fine.to(dev), coarse.to(dev)
    pts = [T(p, dev) for p in frames]
    fresh_workspace()
    coarse_first = coarse(pts, want_stats=True).clone()
    assert coarse.last_stats.num_in[0] == len(ovc_c)
    fresh_workspace()
    a = fine(pts, want_stats=True).clone()
    assert fine.last_stats.num_in[0] == len(ovc_f)
    b = coarse(pts, want_stats=True).clone()
    assert coarse.last_stats.num_in[0] == len(ovc_c)
    c = fine(pts, want_stats=True)
    assert fine.last_stats.num_in[0] == len(ovc_f)
    assert torch.equal(b, coarse_first)
    assert torch.equal(c, a)
    assert (a != 0).any() and (b != 0).any()


@pytest.mark.parametrize("voxel,frames_n,blocks", [(0.6, 5, 99), (0.075, 6, 7594), (0.075, 7, 8860)])
def test_both_scan_paths_rank_like_the_oracle(dev, oracle_mod, voxel, frames_n, blocks):
    """the index scan below kLookBehindBlocks = 8192 scan blocks (every block adds up the totals before it, the last one
    sends the voxel count to the host) and above it (single-workgroup scan, count sent by its own launch): about 100
    blocks, the largest grid below the bound, the smallest above.  Rank order (the sorted voxel coordinates) and the voxel
    count equal the oracle's; the second call on the workspace, with other points, too."""
    side = int(round(108.0 / voxel))
    assert -(-(frames_n * 40 * side * side // 64) // WORDS_PER_SCAN_BLOCK) == blocks
    vs = [voxel, voxel, 0.2]
    lb = make_branch(3, voxel=voxel, side=side) if voxel != VS[0] else make_branch(3)
    calls = [[random_points(100 * frames_n + 10 * call + b, 400, 50.0) for b in range(frames_n)] for call in range(2)]
    want = [oracle_vfe(oracle_mod, lb, frames, vs) for frames in calls]
    vfe = lb.pts_voxel_encoder.to(dev)
    fresh_workspace()
    for frames, (coors, ovf, ovc) in zip(calls, want):
        vf, vc = vfe(T(np.concatenate(frames), dev), T(coors, dev))
        assert len(vc) == len(ovc) and len(ovc) > 300 * frames_n
        assert np.array_equal(vc.cpu().numpy(), ovc)
        assert np.abs(vf.cpu().numpy() - ovf).max() < 1e-4
    fresh_workspace()     # (0.6 GB of maps at seven frames: not kept for the rest of the session)


def test_empty_and_tiny_inputs(dev, oracle_mod):
    """no point in range (N = 0): the stand-alone VFE returns no voxel, the branch refuses the batch, and the next calls
    are right; fewer points than a wave; one voxel of 450 points whose run of records is cut by seven 64-record
    boundaries (its row is zeroed by the mean kernel and accumulated with atomicMax by the layer kernels)"""
    rng = np.random.default_rng(5)
    lb = make_branch(4)
    outside = random_points(31, 500)
    outside[:, 2] = 50.0
    tiny = random_points(32, 37, 3.0)
    long_voxel = np.concatenate([cell_points([(7, 700, 333)], rng, per_cell=450), cell_points([(7, 700, 334)], rng, per_cell=70),
                                 random_points(33, 90, 2.0)])
    long_voxel = long_voxel[rng.permutation(len(long_voxel))]
    want = {k: oracle_vfe(oracle_mod, lb, [v]) for k, v in (("tiny", tiny), ("long", long_voxel))}
    assert np.bincount(np.unique(want["long"][0], axis=0, return_inverse=True)[1].ravel()).max() == 450
    lb = lb.to(dev)
    vfe = lb.pts_voxel_encoder
    first = {}
    for k, v in (("tiny", tiny), ("long", long_voxel)):
        fresh_workspace()
        first[k] = lb([T(v, dev)]).clone()
    fresh_workspace()
    bad_coors = coors_of(oracle_mod, [outside])
    assert (bad_coors[:, 1:] == -1).all()
    for k, v in (("long", long_voxel), ("tiny", tiny), ("long", long_voxel)):
        vf0, vc0 = vfe(T(outside, dev), T(bad_coors, dev))
        assert len(vf0) == 0 and len(vc0) == 0
        with pytest.raises(_lib.IsfError):
            lb([T(outside, dev)])
        coors, ovf, ovc = want[k]
        vf, vc = vfe(T(v, dev), T(coors, dev))
        assert np.array_equal(vc.cpu().numpy(), ovc), k
        err = np.abs(vf.cpu().numpy() - ovf).max()
        assert err < 1e-4, (k, err)
        assert torch.equal(lb([T(v, dev)]), first[k]), k


def test_stand_alone_vfe_twice_on_one_stream(dev, oracle_mod):
    """isf_dynamic_vfe_forward with two point sets, the second touching the first, the last and the words on both sides
    of a scan-block boundary of ITS index (depth 40): the second result equals that call made first, bit for bit"""
    rng = np.random.default_rng(9)
    lb = make_branch(6)
    last = GRID[0] * GRID[1] * GRID[2] // 64 - 1
    one = [random_points(41, 6000), random_points(42, 5000)]
    two = [np.concatenate([cell_points(word_cells(0, GRID[0], 0) + word_cells(1023, GRID[0], 0) + word_cells(1024, GRID[0], 0) +
                                       word_cells(last, GRID[0], 0), rng), random_points(43, 800, 8.0)])]
    coors1 = coors_of(oracle_mod, one)
    coors2, ovf, ovc = oracle_vfe(oracle_mod, lb, two)
    vfe = lb.pts_voxel_encoder.to(dev)
    fresh_workspace()
    vf_first, vc_first = (t.clone() for t in vfe(T(two[0], dev), T(coors2, dev)))
    fresh_workspace()
    vfe(T(np.concatenate(one), dev), T(coors1, dev))
    vf, vc = vfe(T(two[0], dev), T(coors2, dev))
    assert torch.equal(vc, vc_first) and torch.equal(vf, vf_first)
    assert np.array_equal(vc.cpu().numpy(), ovc)
    assert np.abs(vf.cpu().numpy() - ovf).max() < 1e-4
