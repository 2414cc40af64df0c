"""GPU tests of the LiDAR branch's training step as a chain (LidarBranch.forward_train: dynamic voxelize, DynamicVFE's
composed path with DynamicScatter mean / max and their backward, _RowsLinear, the fused bn1d_relu; SparseEncoder's 21
SparseConvFunction layers with fused batch-statistic BatchNorm, residual blocks and dense() with its backward) against the
float64 restatement of tests/lidar_train_common.py, which tests/test_lidar_train.py pins to the CPU oracle.

Bound, the convention of tests/test_gpu_camera_train.py::_within with the whole-module floor made relative: per tensor
err(HIP vs float64) <= 2 x err(the restatement in float32 on the same GPU vs float64) + 1e-4 x max|float64 tensor|.  The
upstream gradient is random, scaled by 1 / sqrt(elements).  Voxel coordinates are oracle.dynamic_voxelize's integers on
both sides; the point clouds hold no near-tie of a per-voxel maximum (asserted on the restatement before any comparison),
so float32 and float64 route every max gradient to the same point, and no ReLU input of the VFE within ten float32
errors of zero.  The encoder's ReLUs cannot be kept clear of zero the same way (a million inputs of order 1): the clouds'
seeds are picked so that the last two levels, where one ReLU that changes side moves a BatchNorm gradient by a tenth, hold
none within the run-to-run spread (lidar_train_common.POINT_SEEDS).

Measured on an MI355X: see DESIGN.md section 4.0c."""
import numpy as np
import pytest
import torch

import lidar_train_common as LT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F64, F32 = torch.float64, torch.float32
FLOOR = 1e-4


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Figures:
    """the bound above for a list of tensors: prints every tensor's figures, then asserts them all"""

    def __init__(self, tag):
        self.tag, self.bad, self.ratio = tag, [], []

    def add(self, name, got, ref, f32, scale=1.0):
        ref = ref.detach().double() * scale
        e_hip = float((got.detach().double() - ref).abs().max())
        e_32 = float((f32.detach().double() * scale - ref).abs().max())
        top = float(ref.abs().max())
        bound = 2 * e_32 + FLOOR * top
        print(f"{self.tag} {name}: max|ref| {top:.3e} err hip {e_hip:.3e} err f32 {e_32:.3e} bound {bound:.3e}")
        self.ratio.append(e_hip / max(e_32, 1e-300))
        if not e_hip <= bound:
            self.bad.append((name, e_hip, e_32, top))

    def check(self):
        r = sorted(self.ratio)
        print(f"{self.tag}: {len(r)} tensors, err hip / err f32 from {r[0]:.2f} to {r[-1]:.2f}, median {r[len(r) // 2]:.2f}")
        assert not self.bad, self.bad


def _upstream(shape, seed=77):
    g = torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)
    return (g / float(np.prod(shape)) ** 0.5).to(DEV)


def _norms(lb):
    return [l.norm for l in lb.pts_voxel_encoder.vfe_layers] + [bn for _, bn in LT.encoder_modules(lb.pts_middle_encoder)]


def _vfe_named(vfe):
    return [(f"vfe {i} {k}", p) for i, l in enumerate(vfe.vfe_layers)
            for k, p in (("weight", l.linear.weight), ("gamma", l.norm.weight), ("beta", l.norm.bias))]


def _enc_named(enc):
    return [(f"conv {i} {k}", p) for i, (c, b) in enumerate(LT.encoder_modules(enc))
            for k, p in (("weight", c.weight), ("gamma", b.weight), ("beta", b.bias))]


def _leaves(params, tag):
    return [(f"{tag} {i} {k}", p[k]) for i, p in enumerate(params) for k in ("weight", "gamma", "beta")]


def _stage_ends(enc):
    """plan-layer index whose output is encode_features[j]: conv_input, then the last conv of every stage"""
    convs = [c for c, _ in LT.encoder_modules(enc)]
    ends = [0]
    for stage in enc.encoder_layers._modules.values():
        ends.append(max(i for i, c in enumerate(convs) if any(c is m for m in stage.modules())))
    return ends


# ----------------------------------------------------------------------------------------------- the whole-branch cases
_CLOUDS, _STEPS, _REFS = {}, {}, {}


def _cloud(second):
    if second not in _CLOUDS:
        pl = LT.point_clouds(LT.POINT_SEEDS[second], second)
        _CLOUDS[second] = (pl, LT.voxelize(pl))
    return _CLOUDS[second]


def _hip_step(second, log2_scale=0):
    """one training step of a freshly seeded LidarBranch from raw points -> its outputs, gradients and BatchNorm buffers"""
    pl, _ = _cloud(second)
    lb = LT.make_branch(LT.MODEL_SEED).to(DEV).train()
    norms = _norms(lb)
    initial = [(bn.running_mean.clone(), bn.running_var.clone()) for bn in norms]
    seen = dict(rows=[])
    hooks = [lb.pts_voxel_encoder.register_forward_hook(lambda m, i, o: seen.update(vc=o[1]))]
    for conv, _ in LT.encoder_modules(lb.pts_middle_encoder):
        hooks.append(conv.register_forward_hook(lambda m, i, o: seen["rows"].append(int(o.features.shape[0]))))
    pts = [_T(p).requires_grad_() for p in pl]
    out = lb(pts)
    out.backward(_upstream(out.shape).float() * 2.0 ** log2_scale)
    for h in hooks:
        h.remove()
    named = _vfe_named(lb.pts_voxel_encoder) + _enc_named(lb.pts_middle_encoder)
    assert all(p.grad is not None for _, p in named)
    return dict(lb=lb, out=out.detach(), vc=seen["vc"], rows=seen["rows"], dpoints=torch.cat([p.grad for p in pts]),
                grads=[(n, p.grad) for n, p in named], initial=initial,
                buffers=[(bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)) for bn in norms])


def _step(second, log2_scale=0):
    if (second, log2_scale) not in _STEPS:
        _STEPS[second, log2_scale] = _hip_step(second, log2_scale)
    return _STEPS[second, log2_scale]


def _reference(second):
    """the same step by the restatement in float64 and in float32, on the GPU; asserts the near-tie precondition (on
    the CPU: lidar_train_common.assert_cloud_has_no_near_ties says why)"""
    if second in _REFS:
        return _REFS[second]
    pl, c4 = _cloud(second)
    lb = LT.make_branch(LT.MODEL_SEED)
    plan = lb.pts_middle_encoder.plan_to_numpy()
    runs, geometry = [], None
    for dt in (F64, F32):
        vp, ep = LT.vfe_params(lb.pts_voxel_encoder, dt, DEV), LT.encoder_params(lb.pts_middle_encoder, dt, DEV)
        pts = _T(np.concatenate(pl)).to(dt).requires_grad_()
        dense, v, rows, stats, geometry = LT.branch_train(plan, vp, ep, pts, _T(c4), len(pl), geometry)
        dense.backward(_upstream(dense.shape).to(dt))
        leaves = _leaves(vp, "vfe") + _leaves(ep, "conv")
        runs.append(dict(out=dense.detach(), v=v, dpoints=pts.grad, grads=[(n, p.grad) for n, p in leaves],
                         stats=v["stats"] + stats, rows=[int(r.shape[0]) for r in rows]))
    LT.assert_cloud_has_no_near_ties(second)
    _REFS[second] = runs
    return runs


def _compare_step(tag, hip, second, log2_scale=0):
    r64, r32 = _reference(second)
    assert torch.equal(hip["vc"].long(), r64["v"]["voxel_coors"])               # voxelize + voxel order from raw points
    assert hip["rows"] == r64["rows"] and min(hip["rows"]) >= 2
    assert tuple(hip["out"].shape) == tuple(r64["out"].shape) == (2, 512, 6, 6)
    fig = _Figures(tag)
    fig.add("map", hip["out"], r64["out"], r32["out"])
    s = 2.0 ** log2_scale
    fig.add("dpoints", hip["dpoints"], r64["dpoints"], r32["dpoints"], s)
    for (n, a), (n64, b), (_, c) in zip(hip["grads"], r64["grads"], r32["grads"]):
        assert n == n64 and a.shape == b.shape
        fig.add("d " + n, a, b, c, s)
    assert len(fig.ratio) == 2 + 3 * 23
    fig.check()
    return fig


@pytest.mark.parametrize("log2_scale", [0, -20])
def test_forward_train_from_raw_points(log2_scale):
    """c: the whole LidarBranch.forward_train from raw points (three of them out of range) and its backward against the
    chained restatement; 2^-20: the upstream gradient at the size a real backward pass carries, through 21 chained
    grad_to_split rescales"""
    hip = _step("blobs", log2_scale)
    _compare_step(f"c 2^{log2_scale}", hip, "blobs", log2_scale)


@pytest.mark.parametrize("second", ["one_voxel", "empty"])
def test_forward_train_with_a_nearly_empty_sample(second):
    """d: sample 1 is a single voxel (one row of its own at every level, down to the last), or holds out-of-range points
    only (every level has rows of sample 0 alone and dense() writes an all-zero sample)"""
    hip = _step(second)
    per_sample = torch.bincount(hip["vc"][:, 0].long(), minlength=2).tolist()
    assert per_sample[0] > 100 and per_sample[1] == (1 if second == "one_voxel" else 0)
    assert float(hip["out"][0].abs().max()) > 0
    assert (float(hip["out"][1].abs().max()) > 0) == (second == "one_voxel")
    _compare_step("d " + second, hip, second)
    pl, c4 = _cloud(second)
    n0 = len(pl[0])
    assert float(hip["dpoints"][:n0].abs().max()) > 0
    if second == "empty":
        assert float(hip["dpoints"][n0:].abs().max()) == 0
    assert float(hip["dpoints"][_T((c4[:, 1:] < 0).any(1))].abs().max()) == 0       # out-of-range points get no gradient


def test_batchnorm_buffers_after_one_step():
    """e: every BatchNorm of the branch (2 in the VFE, 21 in the encoder) after the step of c, from randomised initial
    buffers: num_batches_tracked == 1, and the batch statistic recovered from the buffers, (running - (1 - m) initial) / m
    with m = 0.01, against the restatement's batch mean and UNBIASED batch variance"""
    hip = _step("blobs")
    r64, r32 = _reference("blobs")
    m = LT.MOMENTUM
    fig = _Figures("e")
    assert len(hip["buffers"]) == len(r64["stats"]) == 23
    for i, ((rm, rv, nbt), (rm0, rv0), (mu, var, n, _), (mu32, var32, _, _)) in enumerate(
            zip(hip["buffers"], hip["initial"], r64["stats"], r32["stats"])):
        assert nbt == 1 and n >= 2
        assert float((rm0.abs() > 1e-3).float().mean()) > 0.9 and float((rv0 - 1).abs().max()) > 0.1   # non-trivial start
        fig.add(f"bn {i} mean ({n} rows)", (rm.double() - (1 - m) * rm0.double()) / m, mu, mu32)
        fig.add(f"bn {i} var ({n} rows)", (rv.double() - (1 - m) * rv0.double()) / m, var * (n / (n - 1)), var32 * (n / (n - 1)))
    fig.check()


def test_two_identical_steps():
    """f: a second, identical step of c: the same voxel coordinates and row counts, every output and gradient within the
    bound of the reference again; not bit identity -- the mean scatter sums with float atomics.  Prints the spread."""
    first, second = _step("blobs"), _hip_step("blobs")
    assert torch.equal(first["vc"], second["vc"]) and first["rows"] == second["rows"]
    _compare_step("f first", first, "blobs")
    _compare_step("f second", second, "blobs")
    r64, _ = _reference("blobs")
    worst = 0.0
    for (n, a), (_, b), (_, ref) in [(("map", first["out"]), ("map", second["out"]), ("map", r64["out"])),
                                     (("dpoints", first["dpoints"]), ("", second["dpoints"]), ("", r64["dpoints"]))] + \
            list(zip(first["grads"], second["grads"], r64["grads"])):
        spread, top = float((a.double() - b.double()).abs().max()), float(ref.abs().max())
        worst = max(worst, spread / top)
        print(f"f spread {n}: max|ref| {top:.3e} hip vs hip {spread:.3e} ({spread / top:.2e} of max|ref|)")
    print(f"f: largest run-to-run spread {worst:.2e} of max|ref|")


# ------------------------------------------------------------------------------------------------------- a. VFE alone
def test_vfe_training_step():
    """a: DynamicVFE in train() on the in-range points of the c cloud with the oracle's coordinates: voxel features and
    coordinates, the gradient to the points, both Linear weights and the four BatchNorm affine tensors"""
    pl, c4 = _cloud("blobs")
    keep = (c4[:, 1:] >= 0).all(1)
    pts_np, c4 = np.concatenate(pl)[keep], c4[keep]
    lb = LT.make_branch(LT.MODEL_SEED).to(DEV).train()
    vfe = lb.pts_voxel_encoder
    runs = []
    for dt in (F64, F32):
        vp = LT.vfe_params(vfe, dt, DEV)
        p = _T(pts_np).to(dt).requires_grad_()
        v = LT.vfe_train(vp, p, _T(c4))
        v["voxel_feats"].backward(_upstream(v["voxel_feats"].shape).to(dt))
        runs.append((v, p.grad, _leaves(vp, "vfe")))
    LT.assert_cloud_has_no_near_ties("blobs")
    pts = _T(pts_np).requires_grad_()
    vf, vc = vfe(pts, _T(c4))
    assert vc.dtype == torch.int32 and torch.equal(vc.long(), runs[0][0]["voxel_coors"])
    vf.backward(_upstream(vf.shape).float())
    fig = _Figures("a")
    fig.add("voxel features", vf, runs[0][0]["voxel_feats"], runs[1][0]["voxel_feats"])
    fig.add("dpoints", pts.grad, runs[0][1], runs[1][1])
    for (n, p), (n64, a), (_, b) in zip(_vfe_named(vfe), runs[0][2], runs[1][2]):
        assert n == n64
        fig.add("d " + n, p.grad, a.grad, b.grad)
    assert len(fig.ratio) == 8
    fig.check()


def test_max_scatter_routes_exact_ties_to_the_lowest_point():
    """the clouds above hold no tie by construction, so the convention itself is tested here: DynamicScatter max backward
    on small-integer features (64 voxels of about 60 points, every channel tied many times over) against first_argmax +
    gather, bit for bit"""
    from isfusion_amd.scatter_points import dynamic_scatter
    g = np.random.default_rng(4)
    P, C = 4000, 16
    feats = _T(g.integers(-2, 3, (P, C)).astype(np.float32))
    coors = _T(g.integers(0, 4, (P, 3)).astype(np.int32))
    inv, vcoors, count = LT.voxel_index(torch.cat([torch.zeros_like(coors[:, :1]), coors], 1))
    assert int(count.max()) > 64
    x = feats.clone().requires_grad_()
    red, vc = dynamic_scatter(x, coors, "max")
    key = lambda c: (c[:, 0] * 4 + c[:, 1]) * 4 + c[:, 2]
    order = torch.argsort(key(vc.long()))                       # the kernel's voxel numbering -> sorted (z, y, x)
    assert torch.equal(vc.long()[order], vcoors[:, 1:])
    gout = _upstream(red.shape).float()
    red.backward(gout)
    pf = feats.double().requires_grad_()
    vmax = pf.gather(0, LT.first_argmax(pf.detach(), inv, count)[0])
    assert torch.equal(red.detach()[order].double(), vmax.detach())
    vmax.backward(gout[order].double())
    assert torch.equal(x.grad.double(), pf.grad)
    assert int(((pf.detach() == vmax.detach()[inv]).sum(0) > 4 * len(count)).sum()) == C


# --------------------------------------------------------------------------------------------------- b. encoder alone
def test_encoder_training_step(monkeypatch):
    """b: SparseEncoder.forward_modules in train() on 2458 voxels in blobs with random features: the map, the five
    encode_features, the gradient to the voxel features, 21 conv weights and 42 BatchNorm affine tensors -- with every layer
    on the split-row training path (split forward, dX over the transposed rulebook, f16x3 dW)"""
    from isfusion_amd import spconv
    feats, coors, B = LT.blob_voxels()
    lb = LT.make_branch(LT.MODEL_SEED).to(DEV).train()
    enc = lb.pts_middle_encoder
    plan = enc.plan_to_numpy()
    assert spconv.TRAINING_KERNELS and spconv.WGRAD_F16X3
    assert all(spconv.f16x3_supported(c.in_channels, c.out_channels) for c, _ in LT.encoder_modules(enc))
    runs, geometry = [], None
    for dt in (F64, F32):
        ep = LT.encoder_params(enc, dt, DEV)
        x = _T(feats).to(dt).requires_grad_()
        dense, rows, _, geometry = LT.encoder_train(plan, ep, x, coors, B, geometry=geometry)
        dense.backward(_upstream(dense.shape).to(dt))
        runs.append((dense.detach(), [r.detach() for r in rows], x.grad, _leaves(ep, "conv")))
    calls = []

    def recording(*a, _inner=spconv.split_backward, **k):
        calls.append(a[3])
        return _inner(*a, **k)
    monkeypatch.setattr(spconv, "split_backward", recording)
    x = _T(feats).requires_grad_()
    out, encode = enc.forward_modules(x, _T(coors), B)
    out.backward(_upstream(out.shape).float())
    assert len(calls) == 21                                               # every layer's backward on the split path
    fig = _Figures("b")
    fig.add("map", out, runs[0][0], runs[1][0])
    ends = _stage_ends(enc)
    assert ends == [0, 5, 10, 15, 19] and len(encode) == 5
    print("rows per layer", [r.shape[0] for r in runs[0][1]])
    for j, (t, i) in enumerate(zip(encode, ends)):
        got, idx = LT.sort_rows(t.features, t.indices)
        ref_idx = _T(geometry[i]["out_idx"])
        assert list(t.spatial_shape) == geometry[i]["shape"]
        a, ia = LT.sort_rows(runs[0][1][i], ref_idx)
        b, _ = LT.sort_rows(runs[1][1][i], ref_idx)
        assert torch.equal(idx, ia)
        fig.add(f"encode_features {j} (layer {i}, {a.shape[0]} rows)", got, a, b)
    fig.add("dvoxels", x.grad, runs[0][2], runs[1][2])
    for (n, p), (n64, a), (_, b) in zip(_enc_named(enc), runs[0][3], runs[1][3]):
        assert n == n64
        fig.add("d " + n, p.grad, a.grad, b.grad)
    assert len(fig.ratio) == 1 + 5 + 1 + 63
    fig.check()
