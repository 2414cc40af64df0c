"""The LiDAR branch's input and output passes (-m gpu): frames read in place through isf_lidar_branch_forward_frames, the
BEV map written in two passes (zeros early, occupied segments last), and the level-0 index scan fed by the byte-map pack
pass.  All three are rearrangements of who reads / writes which bytes: every check is bit-exact against the path they
replace (the concatenated entry, ISF_ENC_DIAG_BEV_ONE_PASS) or against the CPU oracle."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# output level [2, 20, 25]: W = 25 is no multiple of 16 or 4, a plane has 500 cells = 15.6 of the 32-cell (128-byte) segments
# the BEV map is cut into, so segments run across row ends, are partial at both ends of a plane and, from the second frame
# on, lie across the 64-bit words of the index
VS = [0.075, 0.075, 0.2]
SHAPE = [41, 160, 200]
RG = [-7.5, -6.0, -5.0, 7.5, 6.0, 3.0]


def test_bev_one_pass_bit_is_named_and_pinned():
    """the diagnostic bit crosses the C ABI as an int: header and _lib agree on 1 << 30, next to the bits tests/test_host.py pins"""
    from isfusion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "isf_hip.h")).read()
    assert re.search(r"^#define ISF_ENC_DIAG_BEV_ONE_PASS \(1 << 30\)", hdr, flags=re.M)
    assert _lib.BEV_ONE_PASS_DIAG == 1073741824
    others = [v for n, v in vars(_lib).items() if n.startswith("ENC_DIAG_") and "VARIANT_SHIFT" not in n]
    assert all(_lib.BEV_ONE_PASS_DIAG & v == 0 for v in others)


def _frame(seed, n, lo=(-8.0, -6.5, -5.5), hi=(8.0, 6.5, 3.5)):
    """n points, uniform in a box a little larger than the range (some fall outside), + intensity, time"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(lo, hi, (n, 3))
    return np.concatenate([xyz, rng.random((n, 2))], 1).astype(np.float32)


@pytest.fixture(scope="module")
def branch(dev):
    import isfusion_amd as m
    me = dict(m.ISFUSION_0075["pts_middle_encoder"])
    me["sparse_shape"] = SHAPE
    lb = m.LidarBranch(voxel_size=VS, point_cloud_range=RG, pts_middle_encoder=me)
    lb = lb.randomize_weights_(0).randomize_bn_(1).eval().to(dev)
    assert lb.pts_middle_encoder.out_channels_and_shape() == (512, 20, 25)
    return lb


def _t(a, dev):
    return torch.from_numpy(a).to(dev)


# ------------------------------------------------------------------------------------------- frames by pointer
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 8])
def test_frames_entry_matches_concatenated_entry(dev, branch, B):
    frames = [_t(_frame(10 + b, 2000 + 377 * b), dev) for b in range(B)]
    got = branch(frames)
    ref = branch(frames, by_pointer=False)
    assert got.shape == (B, 512, 20, 25) and got.abs().max().item() > 0.1
    assert torch.equal(got, ref)


@pytest.mark.gpu
def test_frames_entry_empty_frame_and_offset_view(dev, branch):
    f0, f2 = _frame(31, 3001), _frame(32, 2222)
    empty = torch.empty((0, 5), dtype=torch.float32, device=dev)
    # frame 2 as a view one float into its storage: contiguous rows, base pointer 4-byte aligned only
    store = torch.zeros(1 + f2.size, dtype=torch.float32, device=dev)
    store[1:] = _t(f2, dev).reshape(-1)
    view = store[1:].view(-1, 5)
    assert view.is_contiguous() and view.storage_offset() == 1 and view.data_ptr() % 8 == 4
    frames = [_t(f0, dev), empty, view]
    got = branch(frames)
    ref = branch([_t(f0, dev), empty, _t(f2, dev)], by_pointer=False)
    assert torch.equal(got, ref)
    assert got[1].abs().max().item() == 0 and got[0].abs().max().item() > 0.1 and got[2].abs().max().item() > 0.1


@pytest.mark.gpu
def test_nine_frames_take_the_concatenated_entry(dev, branch):
    frames = [_t(_frame(50 + b, 2000 + 100 * b), dev) for b in range(9)]
    got = branch(frames)                       # more than the frame table holds: concatenated inside forward_eval
    assert got.shape[0] == 9
    first8 = branch(frames[:8])                # frames entry; a frame's map does not depend on its batch
    assert torch.equal(got[:8], first8)
    assert torch.equal(got[8], branch(frames[8:])[0])


# ------------------------------------------------------------------------------------------- two-pass BEV map
def _corner(seed, n):   # every point in one corner of the range: whole lines, and most of every line, stay empty
    return _frame(seed, n, lo=(-7.5, -6.0, -3.0), hi=(-5.5, -4.5, 1.0))


@pytest.mark.gpu
def test_two_pass_bev_matches_one_pass_on_a_reused_buffer(dev, branch):
    from isfusion_amd import _lib
    # frame 1, z = 0 of a 128-byte aligned buffer: the plane starts on a line (float 512 * 500) and at cell 2 * 500 of the
    # index, so its segments are cells 1000 + 32 k ...: every other one lies across a 64-bit word (1000 = 15 * 64 + 40)
    assert (512 * 500) % 32 == 0 and any((1000 + 32 * k) % 64 + 32 > 64 for k in range(15))
    dense = [_t(_frame(70, 5000), dev), _t(_frame(71, 4000), dev)]
    sparse = [_t(_corner(72, 2000), dev), _t(_frame(73, 2500, lo=(-7.5, 1.0, -5.0), hi=(7.5, 1.2, 3.0)), dev)]
    buf = torch.full((2, 512, 20, 25), float("nan"), device=dev)
    for frames in (dense, sparse, [dense[0], sparse[0]]):   # the same buffer: nothing of the previous map may survive
        ref = branch(frames, conv_diag=_lib.BEV_ONE_PASS_DIAG)
        got = branch(frames, out=buf)
        assert got.data_ptr() == buf.data_ptr()
        assert not torch.isnan(buf).any()
        assert torch.equal(buf, ref)
        assert (ref != 0).any()
        buf2 = torch.full_like(buf, float("nan"))
        assert torch.equal(branch(frames, out=buf2, by_pointer=False), ref)
    occupied = (ref[1] != 0).any(0)           # the corner frame: whole y lines of the map are empty
    assert occupied.any() and (~occupied.any(1)).sum().item() >= 10
    # a buffer that is only 4-byte aligned (another cut of the segments, other partial ones at the plane ends) gives the same map
    store = torch.full((1 + buf.numel(),), float("nan"), device=dev)
    odd = store[1:].view_as(buf)
    assert torch.equal(branch(sparse, out=odd), branch(sparse, conv_diag=_lib.BEV_ONE_PASS_DIAG))


@pytest.mark.gpu
def test_two_pass_bev_full_width_rows(dev):
    """W = 180 (a multiple of 4: 16-byte zero stores, a 4-cell segment at the row end) at the benchmark's output shape"""
    import isfusion_amd as m
    from isfusion_amd import _lib, synthetic
    lb = m.LidarBranch().randomize_weights_(0).randomize_bn_(1).eval().to(dev)
    frames = [_t(np.ascontiguousarray(synthetic.lidar_sweeps(90 + b, 4000)), dev) for b in range(2)]
    buf = torch.full((2, 512, 180, 180), float("nan"), device=dev)
    lb(frames, out=buf)
    assert torch.equal(buf, lb(frames, conv_diag=_lib.BEV_ONE_PASS_DIAG))


# ------------------------------------------------------------------------------------------- index scan of the VFE
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2])
def test_vfe_index_scan_from_pack_popcounts(dev, oracle_mod, B):
    """isf_dynamic_vfe_forward on the full 0.075 m grid: 1 266 scan blocks at B = 1 (look-behind prefix launch), 2 532 at
    B = 2 (scanned block sums).  The voxel coordinates come out in rank order, one per occupied cell -- exactly the CPU
    oracle's -- only if the per-block popcounts of the pack pass give the right prefix and total; the features (1e-4: fp32,
    another summation order, as tests/test_gpu_parity.py) only if the per-voxel counters start from zero on a reused
    workspace (second call with other points)."""
    import isfusion_amd as m
    from isfusion_amd import synthetic
    from isfusion_amd.norm import fold_bn
    vs, rg = m.ISFUSION_0075["voxel_size"], m.ISFUSION_0075["point_cloud_range"]
    lb = m.LidarBranch().randomize_weights_(2).randomize_bn_(3).eval()
    vfe = lb.pts_voxel_encoder
    bn1 = [t.numpy() for t in fold_bn(vfe.vfe_layers[0].norm)]
    bn2 = [t.numpy() for t in fold_bn(vfe.vfe_layers[1].norm)]
    w1, w2 = vfe.vfe_layers[0].linear.weight.detach().numpy(), vfe.vfe_layers[1].linear.weight.detach().numpy()
    lb = lb.to(dev)
    for rep in range(2):
        pl = [synthetic.lidar_sweeps(200 + 10 * rep + b, 3000 + 500 * rep) for b in range(B)]
        pts = np.concatenate(pl)
        coors = np.concatenate([np.concatenate([np.full((p.shape[0], 1), b, np.int32),
                                                oracle_mod.dynamic_voxelize(p, vs, rg)], 1) for b, p in enumerate(pl)])
        ovf, ovc, _ = oracle_mod.dynamic_vfe(pts, coors, vs, rg, w1, bn1, w2, bn2)
        vf, vc = lb.pts_voxel_encoder(_t(pts, dev), _t(coors, dev))
        assert vc.shape[0] == ovc.shape[0] and np.array_equal(vc.cpu().numpy(), ovc)
        err = np.abs(vf.cpu().numpy() - ovf).max()
        assert err < 1e-4, err
