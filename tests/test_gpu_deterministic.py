"""GPU tests of the deterministic mode (isfusion_amd.deterministic(); the isf_*_det entries of include/isf_hip.h): the
four kernels that accumulate in 64-bit fixed point -- bit-equal to the numpy restatement of tests/det_common.py, bit-equal
under permutations of their contributions, and inside the existing tests' bounds against float64 -- and whole training
steps that repeat bit for bit (LidarBranch, ISFusionPtsPath in float32 and under bfloat16 autocast, three optimizer
iterations, ISFusionDetector from images).

The step bodies (lidar_steps, path_steps, recipe_runs, detector_steps) take the flag as an argument and return the names
that differed, so that they can also be run with the mode off from a script."""
import random

import numpy as np
import pytest
import torch

import det_common as DC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _det():
    import isfusion_amd
    return isfusion_amd.deterministic()


# ------------------------------------------------------------------------------------------------ A. scatter mean / sum
def _scatter(feats, coors, reduce, det=True):
    import isfusion_amd
    from isfusion_amd import scatter_points as sp
    with isfusion_amd.deterministic(det):
        red, oc, cmap, cnt = sp.dynamic_point_to_voxel_forward(_T(feats), _T(coors), reduce)
    return red.cpu().numpy(), oc.cpu().numpy(), cmap.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("C", [3, 5, 64])
def test_scatter_mean_is_exact_and_order_free(C):
    feats, coors = DC.scatter_case(C)
    P = feats.shape[0]
    ssum, oc, cmap, cnt = _scatter(feats, coors, "sum")
    mean, oc_m, cmap_m, cnt_m = _scatter(feats, coors, "mean")
    M = oc.shape[0]
    assert M == 20 and (cmap < 0).sum() == 40 and cnt.sum() == P - 40
    # 1. bit-equal to the restatement; the mean after its fp32 division
    want = DC.scatter_sum(feats, cmap, M)
    assert ssum.tobytes() == want.tobytes()
    assert mean.tobytes() == (want / cnt[:, None].astype(np.float32)).astype(np.float32).tobytes()
    # 2. a permutation of the rows changes nothing but the order of the map
    perm = np.random.default_rng(C).permutation(P)
    for reduce, ref in (("sum", ssum), ("mean", mean)):
        r2, oc2, cmap2, cnt2 = _scatter(feats[perm], coors[perm], reduce)
        assert r2.tobytes() == ref.tobytes()
        assert np.array_equal(oc2, oc) and np.array_equal(cnt2, cnt) and np.array_equal(cmap2, cmap[perm])
    # 3. the integer outputs are the default entry's
    dmean, doc, dcmap, dcnt = _scatter(feats, coors, "mean", det=False)
    for a, b in ((oc, doc), (oc_m, doc), (cmap, dcmap), (cmap_m, dcmap), (cnt, dcnt), (cnt_m, dcnt)):
        assert np.array_equal(a, b)
    # 4. against float64: the bound tests/test_gpu_parity.py::test_dynamic_scatter_golden_and_oracle applies to the default
    f64 = np.zeros((M, C))
    np.add.at(f64, cmap[cmap >= 0], feats[cmap >= 0].astype(np.float64))
    assert np.allclose(mean, f64 / cnt[:, None], atol=1e-4, rtol=1e-5)
    assert np.allclose(ssum, f64, atol=1e-4, rtol=1e-5)
    # 6. max takes the default's path
    assert _scatter(feats, coors, "max")[0].tobytes() == _scatter(feats, coors, "max", det=False)[0].tobytes()
    # information: how many results the default entry gives on this input
    distinct = {dmean.tobytes()} | {_scatter(feats, coors, "mean", det=False)[0].tobytes() for _ in range(4)}
    print(f"scatter mean C={C}: five calls of the default entry gave {len(distinct)} distinct result(s); "
          f"default == deterministic bits: {dmean.tobytes() == mean.tobytes()}")


def test_scatter_edges():
    rng = np.random.default_rng(5)
    feats = DC.pow2_values(rng, (33, 5))
    coors = rng.integers(0, 4, (33, 3)).astype(np.int32)
    # every row invalid
    bad = coors.copy()
    bad[:, 1] = -1
    red, oc, cmap, cnt = _scatter(feats, bad, "mean")
    assert red.shape == (0, 5) and oc.shape == (0, 3) and cnt.shape == (0,) and (cmap == -1).all()
    # a single row
    red, oc, cmap, cnt = _scatter(feats[:1], coors[:1], "mean")
    assert red.tobytes() == feats[:1].tobytes() and np.array_equal(oc, coors[:1]) and cmap.tolist() == [0] and cnt.tolist() == [1]
    # all zeros
    red, _, _, cnt = _scatter(np.zeros_like(feats), coors, "mean")
    assert red.shape[0] == cnt.shape[0] > 1 and not red.any()
    # one inf: the NaN rule -- every element of the float output, the integer outputs as ever
    inf = feats.copy()
    inf[7, 2] = np.inf
    ok = _scatter(feats, coors, "mean")
    for reduce in ("mean", "sum"):
        red, oc, cmap, cnt = _scatter(inf, coors, reduce)
        assert np.isnan(red).all() and red.shape == ok[0].shape
        assert np.array_equal(oc, ok[1]) and np.array_equal(cmap, ok[2]) and np.array_equal(cnt, ok[3])


# ------------------------------------------------------------------------------------------------ B. P2G backward
def _p2g_grad(case, order=None, det=True):
    import isfusion_amd
    from isfusion_amd import fusion_train as tr
    g = DC.P2G
    pil, coors = case["pillars"], case["pillar_coors"]
    if order is not None:
        pil, coors = pil[order], coors[order]
    img = case["img"].to(DEV).requires_grad_()
    with isfusion_amd.deterministic(det):
        out = tr.p2g_sample(pil.to(DEV), coors.to(DEV), img, case["lidar2img"], case["img_aug"], case["lidar_aug"],
                            g["input_shape"], g["B"], g["bev"], g["cams"])
    out.backward(case["grad_out"].to(DEV))       # outside the block: the Function kept the mode of its forward
    return img.grad.cpu()


@pytest.mark.parametrize("C", [64, 256])
def test_p2g_backward_is_order_free(C):
    from oracle import fusion_ops as orc
    case = DC.p2g_case(C)
    g = DC.P2G
    got = _p2g_grad(case)
    # the case is what it claims: hundreds of taps per cell, border taps, pillars out of view
    ones = dict(case, grad_out=torch.ones_like(case["grad_out"]))
    # per cell the sum of the bilinear weights (0.25 on average per tap): 22 to 204 on the CPU oracle, i.e. a hundred to
    # eight hundred contributions
    weight = _p2g_grad(ones)[:, 0]
    assert weight.min().item() > 20 and weight.numel() == g["B"] * g["cams"] * 15
    # 1. permuting the pillars (rows of pillars and pillar_coors together) changes no bit
    perm = torch.from_numpy(np.random.default_rng(C).permutation(g["pillars"]))
    assert _bits(_p2g_grad(case, perm)) == _bits(got)
    # 2. five calls
    assert all(_bits(_p2g_grad(case)) == _bits(got) for _ in range(4))
    # 3. float64 autograd of the oracle, the bound of tests/test_gpu_train.py::test_p2g_backward_matches_autograd_of_the_restatement
    img = case["img"].double().requires_grad_()
    ref = orc.p2g_sample(case["pillars"].double(), case["pillar_coors"], img, case["lidar2img"].double(),
                         case["img_aug"].double(), case["lidar_aug"].double(), g["input_shape"], g["B"], g["bev"], g["cams"])
    ref.backward(case["grad_out"].double())
    want = img.grad
    assert want.abs().max().item() > 1e-3
    err = (got.double() - want).abs().max().item() / max(1.0, want.abs().max().item())
    print(f"p2g backward C={C}: max|ref| {want.abs().max().item():.3e}, relative error {err:.3e}")
    assert err < 1e-3
    default = _p2g_grad(case, det=False)
    print(f"p2g backward C={C}: default entry == deterministic bits: {_bits(default) == _bits(got)}")
    assert (default.double() - want).abs().max().item() / max(1.0, want.abs().max().item()) < 1e-3


def test_p2g_backward_nan_rule():
    case = DC.p2g_case(64)
    case["grad_out"][1, 3, 2, 2] = float("inf")
    assert torch.isnan(_p2g_grad(case)).all()
    case["grad_out"].zero_()
    assert not _p2g_grad(case).any()


# ------------------------------------------------------------------------------------------------ C. MSDA backward
def _msda_fused(case, perm=None, det=True):
    import isfusion_amd
    from isfusion_amd import fusion_ops as ops
    B, Q, heads, D, P, H, W = case["dims"]
    rows = (lambda t: t) if perm is None else (lambda t: t.view(B, Q, -1)[:, perm].reshape(B * Q, -1))
    v = case["value"].to(DEV).requires_grad_()
    o, lg = rows(case["offsets"]).to(DEV).requires_grad_(), rows(case["logits"]).to(DEV).requires_grad_()
    with isfusion_amd.deterministic(det):
        out = ops.MSDAFunction.apply(v, o, lg, rows(case["ref"]).to(DEV), B, Q, heads, D, P, H, W)
    out.backward(rows(case["grad_out"]).to(DEV))
    return v.grad.cpu(), o.grad.cpu(), lg.grad.cpu()


def test_msda_fused_backward_is_order_free():
    from oracle import fusion_ops as orc
    case = DC.msda_fused_case()
    B, Q, heads, D, P, H, W = case["dims"]
    gv, goff, glog = _msda_fused(case)
    # 1. grad_value after permuting the queries (offsets, logits, ref, grad_output together)
    perm = torch.from_numpy(np.random.default_rng(9).permutation(Q))
    gv2, goff2, glog2 = _msda_fused(case, perm)
    assert _bits(gv2) == _bits(gv)
    assert _bits(goff2) == _bits(goff.view(B, Q, -1)[:, perm].reshape(B * Q, -1))
    # 2. the gradients written once are the default entry's
    dv, doff, dlog = _msda_fused(case, det=False)
    assert _bits(doff) == _bits(goff) and _bits(dlog) == _bits(glog)
    # 3. float64, the bound of tests/test_gpu_widened.py::test_msda_backward_matches_reference_autograd_golden
    v64 = case["value"].double().view(B, H * W, heads, D).requires_grad_()
    o64, l64 = case["offsets"].double().requires_grad_(), case["logits"].double().requires_grad_()
    loc = case["ref"].double().view(B, Q, 1, 1, 1, 2) + o64.view(B, Q, heads, 1, P, 2) / torch.tensor([W, H], dtype=torch.float64)
    outside = ((loc < 0) | (loc > 1)).any(-1).double().mean().item()
    assert 0.05 < outside < 0.95                                        # some samples fall outside the map
    aw = l64.view(B, Q, heads, 1, P).softmax(-1)
    orc.msda_core(v64, torch.tensor([[H, W]]), loc, aw).backward(case["grad_out"].double().view(B, Q, heads * D))
    for name, got, want in (("grad_value", gv, v64.grad.view(B, H * W, heads * D)), ("grad_offsets", goff, o64.grad),
                            ("grad_logits", glog, l64.grad), ("default grad_value", dv, v64.grad.view(B, H * W, heads * D))):
        err, top = (got.double() - want).abs().max().item(), want.abs().max().item()
        print(f"msda fused {name}: max|ref| {top:.3e} err {err:.3e}")
        assert err < 1e-4 * max(1.0, top), name
    # the NaN rule: one inf in grad_output -> every gradient of the call
    bad = dict(case, grad_out=case["grad_out"].clone())
    bad["grad_out"][5, 9] = float("inf")
    assert all(torch.isnan(t).all() for t in _msda_fused(bad))


def _msda_mmcv(case, perm=None, det=True):
    import isfusion_amd
    from isfusion_amd import fusion_ops as ops
    pick = (lambda t: t) if perm is None else (lambda t: t[:, perm].contiguous())
    v = case["value"].to(DEV).requires_grad_()
    loc, aw = pick(case["loc"]).to(DEV).requires_grad_(), pick(case["aw"]).to(DEV).requires_grad_()
    with isfusion_amd.deterministic(det):
        out = ops.ms_deform_attn(v, case["ss"].to(DEV), case["ls"].to(DEV), loc, aw)
    out.backward(pick(case["grad_out"]).to(DEV))
    return v.grad.cpu(), loc.grad.cpu(), aw.grad.cpu()


@pytest.mark.parametrize("D", [16, 12])
def test_msda_mmcv_backward_is_order_free(D):
    """head_dim 16: the location / weight gradients are added once per element (the wave's shuffle tree), only grad_value
    is accumulated; head_dim 12 (no power of two): all three gradients accumulate in fixed point"""
    from oracle import fusion_ops as orc
    case = DC.msda_mmcv_case(D)
    Q = case["loc"].shape[1]
    gv, gl, gw = _msda_mmcv(case)
    perm = torch.from_numpy(np.random.default_rng(D).permutation(Q))
    gv2, gl2, gw2 = _msda_mmcv(case, perm)
    assert _bits(gv2) == _bits(gv)
    assert _bits(gl2) == _bits(gl[:, perm].contiguous()) and _bits(gw2) == _bits(gw[:, perm].contiguous())
    assert all(_bits(a) == _bits(b) for a, b in zip(_msda_mmcv(case), (gv, gl, gw)))
    dv, dl, dw = _msda_mmcv(case, det=False)
    if D == 16:                                                          # written once: the default entry's bits
        assert _bits(dl) == _bits(gl) and _bits(dw) == _bits(gw)
    # float64, the bound of tests/test_gpu_fusion.py::test_ms_deform_attn_with_the_mmcv_signature
    v64, l64, a64 = (t.double().requires_grad_() for t in (case["value"], case["loc"], case["aw"]))
    orc.msda_core(v64, case["ss"], l64, a64).backward(case["grad_out"].double())
    for name, got, want in (("grad_value", gv, v64.grad), ("grad_loc", gl, l64.grad), ("grad_weight", gw, a64.grad),
                            ("default grad_value", dv, v64.grad)):
        err, top = (got.double() - want).abs().max().item(), want.abs().max().item()
        print(f"msda mmcv D={D} {name}: max|ref| {top:.3e} err {err:.3e}")
        assert err < 1e-4 * max(1.0, top), name


# ------------------------------------------------------------------------------------------------ cell gathers
@pytest.mark.parametrize("channels_last", [False, True])
def test_gather_cells_backward_sums_repeated_cells_in_a_fixed_order(channels_last):
    """fusion_ops.gather_cells under the mode (isf_gather_cells_backward): B = 3, 37 cells, 70 entries per sample, so most
    cells are named twice or more and some never; 33 channels (no multiple of the wave).  The forward is torch's gather;
    the gradient equals the float64 index_add within one fp32 sum's rounding (at most 70 terms: 70 x 2^-24 of the row's
    largest magnitude sum), repeats bit for bit, and without repeated cells equals autograd's own bits."""
    import isfusion_amd
    from isfusion_amd import fusion_ops as ops
    B, N, K, E = 3, 37, 70, 33
    g = torch.Generator().manual_seed(12)
    x = torch.randn((B, N, E) if channels_last else (B, E, N), generator=g)
    idx = torch.randint(0, N, (B, K), generator=g)
    idx[0] = 5                                                  # one cell takes every entry of sample 0
    up = torch.randn((B, K, E) if channels_last else (B, E, K), generator=g) * torch.exp2(
        torch.randint(-10, 11, (B, K, 1) if channels_last else (B, 1, K), generator=g).float())

    def run(index, det):
        xd = x.to(DEV).requires_grad_()
        with isfusion_amd.deterministic(det):
            out = ops.gather_cells(xd, index.to(DEV), channels_last)
        out.backward(up.to(DEV))
        return out.detach().cpu(), xd.grad.cpu()

    out, gx = run(idx, True)
    out0, gx0 = run(idx, False)
    assert torch.equal(out, out0)
    assert all(_bits(run(idx, True)[1]) == _bits(gx) for _ in range(3))
    x64 = x.double().requires_grad_()
    dim = 1 if channels_last else 2
    full = idx[:, :, None].expand(-1, -1, E) if channels_last else idx[:, None, :].expand(-1, E, -1)
    x64.gather(dim, full).backward(up.double())
    mag = torch.zeros_like(x64).scatter_add_(dim, full, up.double().abs())
    assert ((gx.double() - x64.grad).abs() <= K * 2.0 ** -24 * mag).all()
    assert ((gx0.double() - x64.grad).abs() <= K * 2.0 ** -24 * mag).all()
    # distinct cells: one gradient per cell, nothing to order -- autograd's bits
    distinct = torch.stack([torch.randperm(N, generator=g)[:30] for _ in range(B)])
    up = up[:, :30] if channels_last else up[:, :, :30]
    assert _bits(run(distinct, True)[1]) == _bits(run(distinct, False)[1])


# ------------------------------------------------------------------------------------------------ D. LidarBranch
def _differ(names_a, names_b):
    """names whose tensors are not torch.equal between two {name: tensor} dicts"""
    assert list(names_a) == list(names_b)
    return [k for k in names_a if not torch.equal(names_a[k], names_b[k])]


def lidar_steps(flag, steps=2):
    import isfusion_amd
    import lidar_train_common as LT
    pl = LT.point_clouds(LT.POINT_SEEDS["blobs"], "blobs")
    assert sum(p.shape[0] for p in pl) == 1200
    runs = []
    for _ in range(steps):
        lb = LT.make_branch(LT.MODEL_SEED).to(DEV).train()
        pts = [_T(p).requires_grad_() for p in pl]
        with isfusion_amd.deterministic(flag):
            out = lb(pts)
        up = torch.randn(out.shape, generator=torch.Generator().manual_seed(77)).to(DEV) / out.numel() ** 0.5
        out.backward(up)
        r = dict(bev=out.detach(), dpoints=torch.cat([p.grad for p in pts]))
        r.update({"grad " + n: p.grad for n, p in lb.named_parameters() if p.grad is not None})
        assert len(r) > 60 and float(r["dpoints"].abs().max()) > 0      # 2 + 21 x 3 conv / norm tensors + the VFE's
        runs.append(r)
    return sorted(set(sum((_differ(runs[0], r) for r in runs[1:]), [])))


def test_lidar_branch_step_repeats_bit_for_bit():
    assert lidar_steps(True) == []


# ------------------------------------------------------------------------------------------------ E / F. the points path
_PATH = {}


def _path():
    if not _PATH:
        from detector_common import build_path, detector_inputs
        from isfusion_amd import head_loss, synthetic
        net = build_path()
        net.pts_bbox_head.train_cfg = dict(head_loss.SHIPPED_TRAIN_CFG)
        net = net.to(DEV)
        pts, inp, kw, metas = detector_inputs()
        scenes = [synthetic.scene_boxes(4321 + i) for i in range(len(pts))]
        _PATH.update(net=net, start={k: v.detach().clone() for k, v in net.state_dict().items()},
                     pts=[_T(p) for p in pts], img=[_T(x) for x in inp["img_feats"]], kw=kw, metas=metas,
                     gtb=[_T(b) for b, _ in scenes], gtl=[_T(l) for _, l in scenes])
    return _PATH


class _rng_restored:
    def __enter__(self):
        self.state = (torch.get_rng_state(), torch.cuda.get_rng_state_all(), random.getstate(), np.random.get_state())

    def __exit__(self, *exc):
        torch.set_rng_state(self.state[0])
        torch.cuda.set_rng_state_all(self.state[1])
        random.setstate(self.state[2])
        np.random.set_state(self.state[3])
        return False


def _fresh(d):
    net = d["net"]
    net.load_state_dict(d["start"], strict=True)
    net.train()
    net.zero_grad(set_to_none=True)
    torch.manual_seed(3)
    random.seed(3)
    np.random.seed(3)
    return net


def _path_step(d, net, autocast):
    leaves = [x.detach().clone().requires_grad_(True) for x in d["img"]]
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        ld = net.forward_train(d["pts"], leaves, d["metas"], d["gtb"], d["gtl"], **d["kw"])
        loss = sum(v.float() for k, v in ld.items() if k != "matched_ious")
    loss.backward()
    return ld, leaves


def path_steps(flag, autocast, steps=3):
    import isfusion_amd
    d = _path()
    runs = []
    with _rng_restored(), isfusion_amd.deterministic(flag):
        for _ in range(steps):
            net = _fresh(d)
            ld, leaves = _path_step(d, net, autocast)
            r = {"loss " + k: v.detach().clone() for k, v in ld.items()}
            assert leaves[1].grad is not None and float(leaves[1].grad.abs().max()) > 0
            r["camera feature gradient"] = leaves[1].grad.clone()
            grads = {"grad " + n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
            assert len(grads) > 100
            r.update(grads)
            runs.append(r)
    print("losses:", {k: float(v) for k, v in runs[0].items() if k.startswith("loss ")})
    return sorted(set(sum((_differ(runs[0], r) for r in runs[1:]), [])))


@pytest.mark.parametrize("autocast", [False, True], ids=["float32", "autocast_bf16"])
def test_points_path_steps_repeat_bit_for_bit(autocast):
    assert path_steps(True, autocast) == []


def recipe_runs(flag, iterations=3):
    import isfusion_amd
    from isfusion_amd.optim import TrainingRecipe
    d = _path()
    finals = []
    with _rng_restored(), isfusion_amd.deterministic(flag):
        for _ in range(2):
            net = _fresh(d)
            recipe = TrainingRecipe.from_config(DC.RECIPE, net, iterations + 1)
            for it in range(iterations):
                recipe.optimizer.zero_grad(set_to_none=True)
                _path_step(d, net, False)
                recipe.step(it)
            torch.cuda.synchronize()
            final = {"model " + k: v.detach().clone() for k, v in net.state_dict().items()}
            for i, st in recipe.optimizer.state_dict()["state"].items():
                final.update({f"optimizer {i} {k}": v.detach().clone() for k, v in st.items() if torch.is_tensor(v)})
            finals.append(final)
    moved = sum(not torch.equal(finals[0]["model " + k], d["start"][k]) for k in d["start"])
    assert moved > 100                                          # the iterations did update the parameters
    return _differ(finals[0], finals[1])


def test_three_recipe_iterations_end_in_the_same_state():
    try:
        assert recipe_runs(True) == []
    finally:
        _PATH.clear()                                           # the path and its inputs: nothing later uses them


# ------------------------------------------------------------------------------------------------ G. from images
def detector_steps(flag, steps=2):
    import isfusion_amd
    import test_gpu_camera_train as TC
    runs = []
    with TC._rng_restored(), isfusion_amd.deterministic(flag):
        try:
            d = TC._detector()
            for _ in range(steps):
                ld, neck, _, _ = TC._detector_step(d)
                r = {"loss " + k: v.detach().clone() for k, v in ld.items()}
                assert len(neck) > 0
                r.update({"img_neck grad " + k: v for k, v in neck.items()})
                runs.append(r)
        finally:
            TC._DET.clear()
    return sorted(set(sum((_differ(runs[0], r) for r in runs[1:]), [])))


def test_detector_step_from_images_repeats_bit_for_bit():
    assert detector_steps(True) == []
