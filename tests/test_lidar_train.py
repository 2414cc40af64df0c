"""CPU pins of tests/lidar_train_common.py, the float64 restatement that tests/test_gpu_lidar_train.py measures the HIP
training step of the LiDAR branch against: eval-mode agreement with the C oracle, the max-scatter gradient convention, the
near-tie precondition of the chosen point clouds, and its own gradients by finite differences."""
import numpy as np
import pytest
import torch

import lidar_train_common as LT

F64, F32, CPU = torch.float64, torch.float32, torch.device("cpu")


@pytest.fixture(scope="module")
def branch():
    return LT.make_branch(LT.MODEL_SEED).eval()


def test_encoder_restatement_equals_the_oracle_in_eval_mode(oracle_mod, branch):
    """folded BatchNorm from the plan: every layer's rows and the dense map against oracle.sparse_encoder_forward.  The
    oracle computes in float32: 21 layers, each a sum of up to 27 x 256 products, a few ulps (6e-8) of the layer's largest
    value per layer -> 2e-5 of the largest value (measured 3e-6)"""
    enc = branch.pts_middle_encoder
    plan = enc.plan_to_numpy()
    feats, coors, B = LT.blob_voxels()
    bev, outs = oracle_mod.sparse_encoder_forward(plan, feats, coors, B)
    with torch.no_grad():
        dense, rows, _, geom = LT.encoder_train(plan, LT.encoder_params(enc, F64, CPU), torch.from_numpy(feats).double(),
                                                coors, B, fold=True)
    assert len(rows) == len(outs) == 21 and tuple(dense.shape) == tuple(bev.shape) == (2, 512, 6, 6)
    print("rows per layer", [r.shape[0] for r in rows])
    assert all(g["out_idx"].shape[0] >= 2 for g in geom)
    for i, (r, o) in enumerate(zip(rows, outs)):
        assert np.array_equal(geom[i]["out_idx"], o[1]) and geom[i]["shape"] == o[2]
        err, top = float((r - torch.from_numpy(o[0]).double()).abs().max()), float(np.abs(o[0]).max())
        assert err <= 2e-5 * top, (i, err, top)
        assert float(r.std(0).min()) > 0, f"layer {i} has a dead channel"
    err, top = float((dense - torch.from_numpy(bev).double()).abs().max()), float(np.abs(bev).max())
    print(f"dense map: max|y| {top:.3e} err {err:.3e}")
    assert err <= 2e-5 * top and top > 1


@pytest.mark.parametrize("second", ["blobs", "one_voxel", "empty"])
def test_vfe_restatement_equals_the_oracle_in_eval_mode(oracle_mod, branch, second):
    """folded BatchNorm: voxel order (sorted (b, z, y, x)) and voxel features against oracle.dynamic_vfe, to the float32
    rounding of the oracle's two 11- and 128-term layers on inputs up to 255: 2e-5 of the largest feature"""
    from isfusion_amd.norm import fold_bn
    vfe = branch.pts_voxel_encoder
    pl = LT.point_clouds(LT.POINT_SEEDS[second], second)
    pts, c4 = np.concatenate(pl), LT.voxelize(pl)
    keep = (c4[:, 1:] >= 0).all(1)
    assert 0 < (~keep).sum() < 8
    fold = [fold_bn(l.norm) for l in vfe.vfe_layers]
    ovf, ovc, _ = oracle_mod.dynamic_vfe(pts, c4, LT.VOXEL_SIZE, LT.PC_RANGE, vfe.vfe_layers[0].linear.weight.detach().numpy(),
                                         [t.numpy() for t in fold[0]], vfe.vfe_layers[1].linear.weight.detach().numpy(),
                                         [t.numpy() for t in fold[1]])
    with torch.no_grad():
        r = LT.vfe_train(LT.vfe_params(vfe, F64, CPU), torch.from_numpy(pts[keep]).double(), torch.from_numpy(c4[keep]),
                         fold=[[t.double() for t in f] for f in fold])
    assert np.array_equal(r["voxel_coors"].numpy(), ovc)
    err, top = float((r["voxel_feats"] - torch.from_numpy(ovf).double()).abs().max()), float(np.abs(ovf).max())
    print(f"{second}: {len(pts)} points, {len(ovc)} voxels, largest {int(r['count'].max())}; max|vf| {top:.3e} err {err:.3e}")
    assert err <= 2e-5 * top and top > 0.5


def test_max_routing_sends_the_gradient_to_the_lowest_tied_point(oracle_mod):
    """first_argmax + gather against oracle.dynamic_scatter_backward on small-integer features: every voxel of several
    points ties exactly in most channels"""
    g = np.random.default_rng(3)
    P, C = 400, 8
    feats = g.integers(-2, 3, (P, C)).astype(np.float32)
    coors = g.integers(0, 4, (P, 3)).astype(np.int32)
    red, _, cmap, cnt = oracle_mod.dynamic_scatter(feats, coors, "max")
    gout = g.normal(size=red.shape).astype(np.float32)
    want = oracle_mod.dynamic_scatter_backward(gout, feats, red, cmap, cnt, "max")
    c4 = torch.from_numpy(np.concatenate([np.zeros((P, 1), np.int32), coors], 1))
    inv, _, count = LT.voxel_index(c4)
    pf = torch.from_numpy(feats).double().requires_grad_()
    arg, _ = LT.first_argmax(pf.detach(), inv, count)
    vmax = pf.gather(0, arg)
    mine = np.zeros(len(count), np.int64)                       # this file's voxel number -> the oracle's
    mine[inv.numpy()] = cmap
    assert np.array_equal(vmax.detach().numpy(), red[mine].astype(np.float64))
    ties = (pf.detach() == vmax.detach()[inv]).long().sum(0)
    assert int((ties > len(count)).sum()) == C                   # more maximal points than voxels: ties in every channel
    (vmax * torch.from_numpy(gout[mine]).double()).sum().backward()
    assert np.array_equal(pf.grad.numpy(), want.astype(np.float64))
    assert not np.array_equal(want, oracle_mod.dynamic_scatter_backward(gout, feats[::-1].copy(), red, cmap[::-1].copy(), cnt,
                                                                        "max")[::-1])   # (the last tied point differs)


@pytest.mark.parametrize("second", ["blobs", "one_voxel", "empty"])
def test_point_clouds_hold_no_near_tie(second):
    """the precondition the GPU tests rest on (and assert again): in the float64 restatement, in both VFE layers, the two
    largest values of every (voxel, channel) with two or more points and a positive maximum lie at least 100 x the largest
    float32 - float64 difference of those values apart, so float32 and float64 route the max gradient to the same point"""
    runs = LT.assert_cloud_has_no_near_ties(second)
    count = runs[0]["count"]
    assert int((count > 64).sum()) >= 2 and int((count == 1).sum()) > 100 and int(((count > 1) & (count <= 30)).sum()) >= 15


def test_encoder_restatement_passes_gradcheck():
    """one SubM layer with an identity residual and one strided layer with the [0, 1, 1] padding, batch-statistic
    BatchNorm, ReLU and the dense map, at about thirty rows in float64"""
    g = np.random.default_rng(11)
    B, shape = 2, [7, 8, 8]
    cells = np.sort(g.choice(B * int(np.prod(shape)), 34, replace=False))
    coors = np.stack(np.unravel_index(cells, (B, *shape)), 1).astype(np.int32)
    plan = dict(sparse_shape=shape, layers=[
        dict(kind="subm", ksize=[3, 3, 3], stride=[1, 1, 1], padding=[1, 1, 1], relu=True, residual_from=-1),
        dict(kind="spconv", ksize=[3, 3, 3], stride=[2, 2, 2], padding=[0, 1, 1], relu=True, residual_from=None)])
    geom = LT.encoder_geometry(plan, coors, B, CPU)
    assert geom[0]["out_idx"].shape[0] == 34 and 8 <= geom[1]["out_idx"].shape[0] < 80
    assert len(geom[0]["taps"]) > 10 and len(geom[1]["taps"]) > 10

    def t(*s, scale=1.0):
        return torch.from_numpy(g.normal(size=s) * scale).requires_grad_()
    x, w0, w1 = t(34, 3), t(3, 3, 3, 3, 3, scale=0.4), t(3, 3, 3, 3, 4, scale=0.4)
    affine = [t(3, scale=0.2), t(3, scale=0.2), t(4, scale=0.2), t(4, scale=0.2)]

    def run(x, w0, w1, g0, b0, g1, b1):
        params = [dict(weight=w0, gamma=1 + g0, beta=b0), dict(weight=w1, gamma=1 + g1, beta=b1)]
        return LT.encoder_train(plan, params, x, coors, B, geometry=geom)[0]
    assert torch.autograd.gradcheck(run, (x, w0, w1, *affine), eps=1e-6, atol=1e-6, rtol=1e-5)
