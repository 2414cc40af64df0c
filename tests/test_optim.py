"""CPU tests of the training recipe's host side (isfusion_amd.optim): mmcv's per-parameter groups on the real model,
the cyclic LR / momentum schedules against a separately written float64 closed form, and the no-fallback rule.  The
recipe's values come from tests/golden/isfusion_0075voxel_train.txt (the evaluated config variables)."""
import ast
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _literal(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return ast.literal_eval(f.read())


@pytest.fixture(scope="module")
def train_cfg():
    return _literal("isfusion_0075voxel_train.txt")


@pytest.fixture(scope="module")
def model_cfg():
    return _literal("isfusion_0075voxel_model.txt")


def test_fixture_holds_the_reference_recipe(train_cfg):
    opt = train_cfg["optimizer"]
    assert opt["type"] == "AdamW" and opt["lr"] == 1e-4 and opt["weight_decay"] == 0.01
    assert opt["paramwise_cfg"] == {"custom_keys": {"img_backbone": {"lr_mult": 0.1}}}
    assert train_cfg["optimizer_config"]["grad_clip"] == {"max_norm": 0.01, "norm_type": 2}
    assert train_cfg["lr_config"]["policy"] == "cyclic" and train_cfg["momentum_config"]["policy"] == "cyclic"


def _check_groups(model, opt, base_lr=1e-4):
    names = [n for n, _ in model.named_parameters()]
    assert len(opt.param_groups) == len(names)
    by_id = {id(p): n for n, p in model.named_parameters()}
    got = [by_id[id(g["params"][0])] for g in opt.param_groups]
    assert got == names                                           # one group per parameter, named_parameters() order
    assert all(len(g["params"]) == 1 for g in opt.param_groups)
    assert all(g["weight_decay"] == pytest.approx(0.01, rel=0, abs=1e-15) for g in opt.param_groups)
    n_img = 0
    for n, g in zip(names, opt.param_groups):
        if n.startswith("img_backbone."):
            n_img += 1
            assert g["lr"] == pytest.approx(base_lr * 0.1, rel=1e-12), n
        else:
            assert g["lr"] == pytest.approx(base_lr, rel=1e-12), n
    return n_img


def test_build_optimizer_pts_path_groups(train_cfg, model_cfg):
    from isfusion_amd import optim, registry
    net = registry.build_pts_path(model_cfg)
    opt = optim.build_optimizer(net, train_cfg["optimizer"])
    assert isinstance(opt, optim.FusedAdamW)
    assert len(opt.param_groups) == 312
    assert _check_groups(net, opt) == 0
    assert sum(p.numel() for g in opt.param_groups for p in g["params"]) == 19209512


def test_build_optimizer_detector_groups(train_cfg, model_cfg):
    from isfusion_amd import optim, registry
    net = registry.build_detector(model_cfg)
    opt = optim.build_optimizer(net, train_cfg["optimizer"])
    assert len(opt.param_groups) == 499
    assert _check_groups(net, opt) == 175


def test_build_optimizer_paramwise_rules():
    """longest custom key first (ties alphabetical), decay_mult, bias multipliers on non-norm biases only, frozen
    parameters kept as plain groups, unsupported options raise"""
    from isfusion_amd import optim
    net = torch.nn.Sequential()
    net.add_module("ab", torch.nn.Linear(2, 2))
    net.add_module("abc", torch.nn.Linear(2, 2))
    net.add_module("bn", torch.nn.BatchNorm1d(2))
    net.add_module("frozen", torch.nn.Linear(2, 2))
    net.frozen.weight.requires_grad_(False)
    cfg = dict(type="AdamW", lr=1.0, weight_decay=0.5,
               paramwise_cfg=dict(custom_keys={"ab": dict(lr_mult=2.0), "abc": dict(lr_mult=3.0, decay_mult=0.0)},
                                  bias_lr_mult=5.0, bias_decay_mult=0.25))
    opt = optim.build_optimizer(net, cfg)
    g = {n: grp for (n, _), grp in zip(net.named_parameters(), opt.param_groups)}
    assert g["ab.weight"]["lr"] == 2.0 and g["ab.bias"]["lr"] == 2.0 and g["ab.weight"]["weight_decay"] == 0.5
    assert g["abc.weight"]["lr"] == 3.0 and g["abc.weight"]["weight_decay"] == 0.0
    assert g["bn.bias"]["lr"] == 1.0 and g["bn.bias"]["weight_decay"] == 0.5           # norm bias: no bias mult
    assert g["frozen.bias"]["lr"] == 5.0 and g["frozen.bias"]["weight_decay"] == 0.125
    assert g["frozen.weight"]["lr"] == 1.0 and g["frozen.weight"]["weight_decay"] == 0.5   # frozen: defaults
    single = optim.build_optimizer(net, dict(type="AdamW", lr=1e-3))
    assert len(single.param_groups) == 1 and len(single.param_groups[0]["params"]) == 8
    for bad in (dict(norm_decay_mult=0.0), dict(dwconv_decay_mult=0.0), dict(bypass_duplicate=True)):
        with pytest.raises(NotImplementedError):
            optim.build_optimizer(net, dict(type="AdamW", lr=1e-3, paramwise_cfg=bad))
    with pytest.raises(NotImplementedError):
        optim.build_optimizer(net, dict(type="SGD", lr=1e-3))
    for bad in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True)):
        with pytest.raises(NotImplementedError):
            optim.FusedAdamW(net.parameters(), **bad)


def _closed_form(base, r0, r1, max_iters, step_ratio_up, it):
    """mmcv's cyclic schedule (cyclic_times 1, gamma 1, cos annealing) written out in float64"""
    period = max_iters
    up = int(step_ratio_up * period)
    i = it % period
    if i < up:
        a, b, f = base, base * r0, i / up
    else:
        a, b, f = base * r0, base * r1, (i - up) / (period - up)
    return b + 0.5 * (a - b) * (1.0 + math.cos(math.pi * f))


@pytest.mark.parametrize("max_iters", [1000, 7])
def test_cyclic_lr_and_momentum_schedules(train_cfg, max_iters):
    from isfusion_amd import optim
    lr_cfg, mom_cfg = train_cfg["lr_config"], train_cfg["momentum_config"]
    lr_up = optim.CyclicLrUpdater(lr_cfg, max_iters)
    mom_up = optim.CyclicMomentumUpdater(mom_cfg, max_iters)
    p1, p2 = torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(2))
    opt = torch.optim.AdamW([dict(params=[p1], lr=1e-4), dict(params=[p2], lr=1e-5)], betas=(0.9, 0.999))
    U = int(0.4 * max_iters)
    for it in (0, 1, U - 1, U, U + 1, max_iters - 1):
        lr_up.before_train_iter(opt, it)
        mom_up.before_train_iter(opt, it)
        for g, base in zip(opt.param_groups, (1e-4, 1e-5)):
            assert g["initial_lr"] == base and g["initial_momentum"] == 0.9
            want_lr = _closed_form(base, 10, 1e-4, max_iters, 0.4, it)
            want_m = _closed_form(0.9, 0.8947368421052632, 1, max_iters, 0.4, it)
            assert g["lr"] == pytest.approx(want_lr, rel=1e-12, abs=0)
            assert g["betas"][0] == pytest.approx(want_m, rel=1e-12, abs=0) and g["betas"][1] == 0.999
        if it == 0:
            assert opt.param_groups[0]["lr"] == pytest.approx(1e-4, rel=1e-12)
            assert opt.param_groups[0]["betas"][0] == pytest.approx(0.9, rel=1e-12)
        if it == U:
            assert opt.param_groups[0]["lr"] == pytest.approx(1e-3, rel=1e-12)
            assert opt.param_groups[0]["betas"][0] == pytest.approx(0.9 * 0.8947368421052632, rel=1e-12)
    with pytest.raises(NotImplementedError):
        optim.CyclicLrUpdater(dict(policy="step", step=[8]), max_iters)


def test_recipe_from_config_dict(train_cfg):
    from isfusion_amd import optim
    net = torch.nn.Linear(3, 2)
    r = optim.TrainingRecipe.from_config(train_cfg, net, max_iters=100)
    assert isinstance(r.optimizer, optim.FusedAdamW) and len(r.optimizer.param_groups) == 2
    assert r.grad_clip == {"max_norm": 0.01, "norm_type": 2}
    assert r.lr_updater.up == 40 and r.momentum_updater.period == 100
    with pytest.raises(NotImplementedError):
        optim.TrainingRecipe.from_config(dict(train_cfg, optimizer_config=dict(grad_clip=dict(max_norm=1, norm_type=1))),
                                         net, 100)


def test_fused_adamw_refuses_cpu_tensors():
    from isfusion_amd import optim
    from isfusion_amd._lib import IsfError
    p = torch.nn.Parameter(torch.ones(5))
    p.grad = torch.full((5,), 0.5)
    opt = optim.FusedAdamW([p], lr=1e-3)
    with pytest.raises(IsfError):
        opt.step()
    with pytest.raises(IsfError):
        opt.step(grad_clip=dict(max_norm=0.01, norm_type=2))
    with pytest.raises(IsfError):
        optim.clip_grad_norm_([p], 0.01)
    assert torch.equal(p.detach(), torch.ones(5))                # nothing was updated on the host
