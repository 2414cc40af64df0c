"""FusedAdamW / clip_grad_norm_ / TrainingRecipe on the GPU (is-fusion_amd/optim.py, csrc/isf_optim.hip): parity with
torch.optim.AdamW + torch.nn.utils.clip_grad_norm_ run in float64, bitwise determinism, awkward sizes and gradient
layouts (DDP bucket views at odd 4-byte offsets), state_dict interchange with torch.optim.AdamW, the modules' packed-
weight caches after a fused step, and the launch budget (2 kernels, no copy, no sync per clipped step)."""
import ast
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_NORM = 0.01


def _train_cfg():
    with open(os.path.join(HERE, "golden", "isfusion_0075voxel_train.txt")) as f:
        return ast.literal_eval(f.read())


@pytest.fixture(scope="module")
def pts_net(dev):
    from isfusion_amd.detector import ISFusionPtsPath
    torch.manual_seed(0)
    return ISFusionPtsPath().to(dev)


def _fused_on_clones(net, cfg):
    """FusedAdamW with build_optimizer's groups of `net`, over fresh clones of its parameters"""
    from isfusion_amd import optim
    proto = optim.build_optimizer(net, cfg)
    params = [p.detach().clone().requires_grad_() for p in net.parameters()]
    groups = [dict({k: v for k, v in g.items() if k != "params"}, params=[q]) for g, q in zip(proto.param_groups, params)]
    return optim.FusedAdamW(groups, **{k: v for k, v in cfg.items() if k not in ("type", "paramwise_cfg")}), params


def _torch_double_twin(opt):
    """torch.optim.AdamW(foreach=False) over float64 copies, same groups / hyperparameters"""
    params, groups = [], []
    for g in opt.param_groups:
        qs = [p.detach().double().clone().requires_grad_() for p in g["params"]]
        params += qs
        groups.append(dict(params=qs, lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"]))
    return torch.optim.AdamW(groups, foreach=False), params


def _grads(params, step, dev, scale):
    """seeded gradients; every 7th tensor (rotating) has none on odd steps"""
    gen = torch.Generator(device=dev).manual_seed(1000 + step)
    out = []
    for i, p in enumerate(params):
        if step % 2 == 1 and (i + step) % 7 == 0:
            out.append(None)
        else:
            out.append(torch.randn(p.shape, generator=gen, device=dev) * scale)
    return out


SCALES = [1.0, 3e-2, 1e-9, 10.0, 1e-3]   # step 2: norm ~ 4e-6 < max_norm -> coef 1


def _run_parity(net, dev, steps, max_iters=50, with_ref=True):
    from isfusion_amd import optim
    cfg = _train_cfg()
    fused, params = _fused_on_clones(net, cfg["optimizer"])
    ref, rparams = _torch_double_twin(fused) if with_ref else (None, None)
    up = [optim.CyclicLrUpdater(cfg["lr_config"], max_iters), optim.CyclicMomentumUpdater(cfg["momentum_config"], max_iters)]
    up_ref = [optim.CyclicLrUpdater(cfg["lr_config"], max_iters),
              optim.CyclicMomentumUpdater(cfg["momentum_config"], max_iters)]
    acc_lr = torch.zeros(len(params), dtype=torch.float64)
    norms, ref_norms = [], []
    for s in range(steps):
        gs = _grads(params, s, dev, SCALES[s % len(SCALES)])
        for p, g in zip(params, gs):
            p.grad = g
        for u in up:
            u.before_train_iter(fused, s)
        fused.step(grad_clip=dict(max_norm=MAX_NORM, norm_type=2))
        norms.append(fused.last_grad_norm.clone())
        if ref is not None:
            for q, g in zip(rparams, gs):
                q.grad = None if g is None else g.double()
            for u in up_ref:
                u.before_train_iter(ref, s)
            ref_norms.append(float(torch.nn.utils.clip_grad_norm_([q for q in rparams if q.grad is not None], MAX_NORM)))
            ref.step()
            for i, (g, grp) in enumerate(zip(gs, ref.param_groups)):
                if g is not None:
                    acc_lr[i] += grp["lr"]
    return fused, params, ref, rparams, acc_lr, [float(n) for n in norms], ref_norms


def test_parity_with_torch_adamw_and_clip_in_float64(pts_net, dev):
    """20 steps on the real 312-tensor, 19.2 M parameter set: mmcv groups, cyclic lr / momentum (max_iters 50), clip
    at 0.01, gradients at several scales (one step under max_norm), some gradients None on some steps"""
    fused, params, ref, rparams, acc_lr, norms, ref_norms = _run_parity(pts_net, dev, 20)
    assert len(params) == 312 and sum(p.numel() for p in params) == 19209512
    assert ref_norms[2] < MAX_NORM and all(n > MAX_NORM for i, n in enumerate(ref_norms) if i % 5 != 2)
    for n, r in zip(norms, ref_norms):
        assert abs(n - r) <= 2e-6 * r, (n, r)
    worst = 0.0
    for i, (p, q) in enumerate(zip(params, rparams)):
        err = float((p.detach().double() - q.detach()).abs().max())
        # Adam's m / sqrt(v) is ill-conditioned where |g| is near eps, so the error is measured against the accumulated
        # update (~ lr per element per step), plus fp32 rounding of |p| over the steps
        tol = 1e-3 * float(acc_lr[i]) + 20 * 2.5e-7 * (1.0 + float(q.detach().abs().max()))
        worst = max(worst, err / tol)
        assert err <= tol, (i, err, tol)
    st = fused.state[params[0]]
    assert float(st["step"]) == float(ref.state[rparams[0]]["step"])
    print(f"\nfused AdamW + clip vs float64 torch: worst error / tolerance {worst:.3f}, norms {norms[:3]}")


def test_coef_one_leaves_update_unscaled(dev):
    """a step whose norm is under max_norm: the fused step equals the unclipped one bit for bit"""
    from isfusion_amd import optim
    torch.manual_seed(3)
    base = [torch.randn(n, device=dev) for n in (5, 70000)]
    grads = [torch.randn(n, device=dev) * 1e-7 for n in (5, 70000)]
    outs = []
    for clip in (None, dict(max_norm=MAX_NORM)):
        ps = [b.clone().requires_grad_() for b in base]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt = optim.FusedAdamW(ps, lr=1e-3)
        opt.step(grad_clip=clip)
        outs.append([p.detach().clone() for p in ps])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_bitwise_determinism(pts_net, dev):
    a = _run_parity(pts_net, dev, 4, with_ref=False)
    b = _run_parity(pts_net, dev, 4, with_ref=False)
    assert a[5] == b[5]
    for p, q in zip(a[1], b[1]):
        assert torch.equal(p, q)
        sa, sb = a[0].state[p], b[0].state[q]
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])


SIZES = (0, 1, 3, 1023, 65537, 40000)


def _awkward_set(dev, seed):
    """parameters of the awkward sizes (one a view at an odd offset of a flat buffer) and gradients that are views at
    odd 4-byte offsets of one flat buffer -- DDP's gradient_as_bucket_view layout"""
    torch.manual_seed(seed)
    ps = [torch.randn(n, device=dev).requires_grad_() for n in SIZES[:-1]]
    flat_p = torch.randn(SIZES[-1] + 1, device=dev)
    ps.append(flat_p[1:].requires_grad_())
    bucket = torch.zeros(sum(SIZES) + 2 * len(SIZES) + 1, device=dev)
    grads, off = [], 1
    for n in SIZES:
        grads.append(bucket[off:off + n])
        off += n + 2
    return ps, bucket, grads


def test_awkward_sizes_and_bucket_view_gradients(dev):
    from isfusion_amd import optim
    ps, bucket, grads = _awkward_set(dev, 5)
    assert any(g.data_ptr() % 16 for g in grads)
    groups = [dict(params=[p], lr=1e-3 * (1 + i)) for i, p in enumerate(ps)]
    opt = optim.FusedAdamW(groups, weight_decay=0.05)
    rq = [p.detach().double().clone().requires_grad_() for p in ps]
    ref = torch.optim.AdamW([dict(params=[q], lr=1e-3 * (1 + i)) for i, q in enumerate(rq)], weight_decay=0.05,
                            foreach=False)
    for p, g in zip(ps, grads):
        p.grad = g
    gen = torch.Generator(device=dev).manual_seed(9)
    for s in range(4):
        bucket.copy_(torch.randn(bucket.shape, generator=gen, device=dev))
        opt.step(grad_clip=dict(max_norm=0.5))
        for q, g in zip(rq, grads):
            q.grad = g.double()
        rn = float(torch.nn.utils.clip_grad_norm_(rq, 0.5))
        ref.step()
        assert abs(float(opt.last_grad_norm) - rn) <= 2e-6 * rn
    for i, (p, q) in enumerate(zip(ps, rq)):
        assert p.numel() == SIZES[i]
        if p.numel():
            err = float((p.detach().double() - q.detach()).abs().max())
            assert err <= 1e-3 * 4 * 1e-3 * (1 + i) + 1e-6, (i, err)
    assert float(opt.state[ps[0]]["step"]) == 4.0


def test_more_hyperparameter_tuples_than_kernel_arguments(dev):
    """20 groups with distinct lr: the tuples go to the device instead of the kernel arguments"""
    from isfusion_amd import optim
    torch.manual_seed(11)
    ps = [torch.randn(300 + i, device=dev).requires_grad_() for i in range(20)]
    rq = [p.detach().double().clone().requires_grad_() for p in ps]
    opt = optim.FusedAdamW([dict(params=[p], lr=1e-4 * (i + 1)) for i, p in enumerate(ps)])
    ref = torch.optim.AdamW([dict(params=[q], lr=1e-4 * (i + 1)) for i, q in enumerate(rq)], foreach=False)
    for s in range(3):
        for p, q in zip(ps, rq):
            p.grad = torch.randn_like(p)
            q.grad = p.grad.double()
        opt.step()
        ref.step()
    for i, (p, q) in enumerate(zip(ps, rq)):
        assert float((p.detach().double() - q.detach()).abs().max()) <= 3e-3 * 1e-4 * (i + 1) + 1e-6


def _small_set(dev, seed=21):
    torch.manual_seed(seed)
    return [torch.randn(n, device=dev).requires_grad_() for n in (7, 4096, 33000)]


def _feed(ps, s, dev):
    gen = torch.Generator(device=dev).manual_seed(500 + s)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=gen, device=dev)


@pytest.mark.parametrize("first", ["fused", "torch"])
def test_state_dict_interchange_with_torch_adamw(dev, first):
    """5 steps of one optimizer, state_dict into the other, 5 more == 10 steps of the fused optimizer"""
    from isfusion_amd import optim
    kw = dict(lr=1e-3, weight_decay=0.02, betas=(0.85, 0.99))
    make = {"fused": lambda ps: optim.FusedAdamW(ps, **kw), "torch": lambda ps: torch.optim.AdamW(ps, foreach=False, **kw)}
    second = "torch" if first == "fused" else "fused"
    ps_a = _small_set(dev)
    a = make[first](ps_a)
    for s in range(5):
        _feed(ps_a, s, dev)
        a.step()
    b = make[second](ps_a)
    b.load_state_dict(a.state_dict())
    for s in range(5, 10):
        _feed(ps_a, s, dev)
        b.step()
    ps_r = _small_set(dev)
    r = optim.FusedAdamW(ps_r, **kw)
    for s in range(10):
        _feed(ps_r, s, dev)
        r.step()
    for p, q in zip(ps_a, ps_r):
        assert float((p - q).detach().abs().max()) <= 1e-4 * 10 * 1e-3 + 1e-6 * (1.0 + float(q.abs().max()))
    sd = b.state_dict()
    assert float(sd["state"][0]["step"]) == 10.0 and sd["state"][0]["step"].dtype == torch.float32
    assert not sd["state"][0]["step"].is_cuda


def test_packed_weight_caches_follow_the_fused_step(dev):
    """the training path's packed-filter caches (sparse-conv forward / dX pairs, dense 3x3 conv groups) detect weight
    changes through Tensor._version only: after 2 fused steps the caches must pack the stepped weights anew (they hand
    out the stale packs when the step does not bump the versions)"""
    from detector_common import build_path
    from isfusion_amd import dense_train, optim, spconv
    net = build_path().to(dev).train()
    sw = next(m.weight for m in net.pts_middle_encoder.modules()
              if isinstance(m, spconv.SubMConv3d) and spconv.f16x3_supported(m.weight.shape[-2], m.weight.shape[-1]))
    dw = next(m.weight for m in net.modules() if dense_train.supported(m))

    def spack():
        K = int(torch.tensor(sw.shape[:-2]).prod())
        return list(spconv._packed_pair(sw, sw.detach().float().contiguous(), K, sw.shape[-2], sw.shape[-1]))

    def dpack():
        return [t for grp in dense_train._groups(dw, False) for t in grp[2:]]

    stale = spack() + dpack()                                    # fills both caches
    assert all(a is b for a, b in zip(stale, spack() + dpack()))  # unchanged weights: the cached packs come back
    versions = (sw._version, dw._version)
    opt = optim.FusedAdamW([sw, dw], lr=1e-2)
    for s in range(2):
        sw.grad, dw.grad = torch.randn_like(sw), torch.randn_like(dw)
        opt.step(grad_clip=dict(max_norm=MAX_NORM))
    assert sw._version > versions[0] and dw._version > versions[1]
    assert not any(a is b for a, b in zip(stale, spack() + dpack()))   # stepped weights: packed anew


def test_launch_budget_and_no_sync(pts_net, dev):
    """steady state (gradients kept between steps, as DDP bucket views are): one clipped step over 312 tensors in 312
    groups is <= 2 kernels and no memcpy, with no host sync"""
    from torch.profiler import ProfilerActivity, profile
    opt, params = _fused_on_clones(pts_net, _train_cfg()["optimizer"])
    gen = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen, device=dev)
    clip = dict(max_norm=MAX_NORM, norm_type=2)
    for _ in range(2):
        opt.step(grad_clip=clip)
    torch.cuda.synchronize()

    def gpu_ops(fn):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and not e.name.startswith("Optimizer.")]                # the step's annotation on the GPU timeline
        copies = [e.name for e in evs if "memcpy" in e.name.lower() or "copy" in e.name.lower()]
        return [e.name for e in evs if e.name not in copies], copies

    kernels, copies = gpu_ops(lambda: opt.step(grad_clip=clip))
    assert 1 <= len(kernels) <= 2 and not copies, (kernels, copies)
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step(grad_clip=clip)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    ref = torch.optim.AdamW([dict(params=[p], lr=1e-4, weight_decay=0.01) for p in params])
    ref.step()

    def stock():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        ref.step()
    k2, c2 = gpu_ops(stock)
    print(f"\nlaunches per clipped step: fused {len(kernels)} (+{len(copies)} copies), torch AdamW(foreach) + "
          f"clip_grad_norm_ on 312 groups {len(k2)} (+{len(c2)} copies)")


def test_standalone_clip_grad_norm_matches_torch(dev):
    from isfusion_amd import optim
    ps, bucket, grads = _awkward_set(dev, 8)
    for p, g in zip(ps, grads):
        p.grad = g
    torch.manual_seed(2)
    bucket.copy_(torch.randn(bucket.shape, device=dev) * 0.3)
    rq = [p.detach().double().clone().requires_grad_() for p in ps]
    for q, g in zip(rq, grads):
        q.grad = g.double()
    n_ref = float(torch.nn.utils.clip_grad_norm_(rq, 0.05))
    n = optim.clip_grad_norm_(ps, 0.05)
    assert n.is_cuda and abs(float(n) - n_ref) <= 2e-6 * n_ref
    for p, q in zip(ps, rq):
        if p.numel():
            assert float((p.grad.double() - q.grad).abs().max()) <= 1e-6 * float(q.grad.abs().max()) + 1e-12
    before = [p.grad.clone() for p in ps]
    n2 = optim.clip_grad_norm_(ps, 10.0)                         # under the limit: gradients untouched
    assert float(n2) <= 10.0 and all(torch.equal(a, p.grad) for a, p in zip(before, ps))


def test_training_recipe_end_to_end(dev):
    """3 steps of ISFusionPtsPath with TrainingRecipe.from_config and the stand-in loss: finite losses and norms, and
    torch AdamW + clip applied to clones of the same gradients gives the same parameters"""
    from detector_common import build_path, detector_inputs
    from isfusion_amd import optim
    net = build_path().to(dev).train()
    for p in net.pts_bbox_head.parameters():
        p.requires_grad_(False)                                  # the stand-in loss does not reach the head
    pts, inp, kw, metas = detector_inputs()
    pts = [torch.from_numpy(p).to(dev) for p in pts]
    img = tuple(torch.from_numpy(a).to(dev) for a in inp["img_feats"])
    cfg = _train_cfg()
    recipe = optim.TrainingRecipe.from_config(cfg, net, max_iters=10)
    names = [n for n, _ in net.named_parameters()]
    twin_params = [p.detach().clone().requires_grad_() for p in net.parameters()]
    twin = torch.optim.AdamW([dict(params=[q], lr=g["lr"], weight_decay=g["weight_decay"])
                              for q, g in zip(twin_params, recipe.optimizer.param_groups)], foreach=False)
    ups = [optim.CyclicLrUpdater(cfg["lr_config"], 10), optim.CyclicMomentumUpdater(cfg["momentum_config"], 10)]
    acc = 0.0
    for it in range(3):
        out, hm = net.forward_train_pts(pts, img, metas, **kw)
        loss = (out[0] ** 2).mean() + hm.sigmoid().mean()
        recipe.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        assert torch.isfinite(loss)
        for q, (n, p) in zip(twin_params, net.named_parameters()):
            q.grad = None if p.grad is None else p.grad.clone()
        norm = recipe.step(it)
        assert torch.isfinite(norm) and float(norm) > 0
        for u in ups:
            u.before_train_iter(twin, it)
        tn = torch.nn.utils.clip_grad_norm_([q for q in twin_params if q.grad is not None], MAX_NORM)
        assert abs(float(norm) - float(tn)) <= 1e-5 * float(tn)
        twin.step()
        acc += twin.param_groups[0]["lr"]
    for n, p, q in zip(names, net.parameters(), twin_params):
        err = float((p.detach() - q.detach()).abs().max())
        assert err <= 2e-3 * acc + 1e-6 * (1 + float(q.detach().abs().max())), (n, err)
