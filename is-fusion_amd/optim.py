"""The reference's training recipe on HIP: AdamW with global-norm gradient clipping and the cyclic LR / momentum schedules
(configs/isfusion/isfusion_0075voxel.py:398-413, wired up by mmdet3d/apis/train.py:92,121-132 through mmcv 1.4).

build_optimizer       mmcv's DefaultOptimizerConstructor: with `paramwise_cfg` one param group per parameter (custom_keys,
                      bias_lr_mult / bias_decay_mult), else a single group.
FusedAdamW            torch.optim.AdamW's interface, parameter-group semantics and state layout (its state_dict loads
                      into torch.optim.AdamW and back), but the whole step -- clip included -- is two HIP launches
                      (isf_optim_grad_sumsq + isf_optim_adamw, csrc/isf_optim.hip) whatever the number of tensors or groups.
clip_grad_norm_       torch.nn.utils.clip_grad_norm_ (norm_type 2) in the same two launches; returns the device norm.
CyclicLrUpdater,      mmcv's CyclicLrUpdaterHook / CyclicMomentumUpdaterHook (by_epoch=False): set each group's `lr` and
CyclicMomentumUpdater `betas[0]` before an iteration.
TrainingRecipe        the three above from the config: mmcv's LR / momentum hooks + OptimizerHook for one iteration.

There is no fallback: CPU, non-fp32, non-contiguous or sparse parameters / gradients raise IsfError."""
import math

import numpy as np
import torch
from torch import nn

from . import _lib
from ._lib import IsfError

CHUNK = _lib.OPTIM_CHUNK


# ------------------------------------------------------------------------------------------------ device tables
class _Plan:
    """The device tensor / chunk table of one set of tensors (int64 [T, 6] = p, g, m, v, numel, hp index, then int32
    [C, 2] = tensor, chunk), the fp64 partial sums and the fp32 norm scalar.  The table is re-uploaded -- from a pinned
    buffer, an event guarding its reuse -- only when a pointer, a numel or a tuple index changes."""

    def __init__(self, device):
        self.device = device
        self.key = None
        self.num_chunks = 0
        self.table = self.pinned = self.event = None
        self.partials = None
        self.norm = torch.zeros((), dtype=torch.float32, device=device)
        self.hp_dev = self.hp_pinned = self.hp_event = None

    def update(self, key, entries):
        if key == self.key:
            return
        t = len(entries)
        counts = np.array([(e[4] + CHUNK - 1) // CHUNK for e in entries], np.int64)
        c = int(counts.sum())
        words = 6 * t + c
        host = np.zeros(max(words, 1), np.int64)
        if t:
            host[:6 * t] = np.array(entries, np.int64).reshape(-1)
        ch = host[6 * t:6 * t + c].view(np.int32).reshape(c, 2)
        ch[:, 0] = np.repeat(np.arange(t, dtype=np.int32), counts)
        starts = np.repeat(np.cumsum(counts) - counts, counts)
        ch[:, 1] = np.arange(c, dtype=np.int64) - starts
        if self.pinned is None or self.pinned.numel() < host.size:
            self.pinned = torch.empty(host.size, dtype=torch.int64, pin_memory=True)
            self.table = torch.empty(host.size, dtype=torch.int64, device=self.device)
            self.event = None
        if self.event is not None:
            self.event.synchronize()                 # the previous upload has left the pinned buffer
        self.pinned[:host.size].numpy()[:] = host
        self.table[:host.size].copy_(self.pinned[:host.size], non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()
        if self.partials is None or self.partials.numel() < max(c, 1):
            self.partials = torch.empty(max(c, 1), dtype=torch.float64, device=self.device)
        self.num_tensors, self.num_chunks, self.key = t, c, key

    def pointers(self):
        base = self.table.data_ptr()
        return base, base + 8 * 6 * self.num_tensors

    def hp_device(self, hps):
        """upload hyperparameter tuples beyond the kernel-argument limit (rare: > 16 distinct tuples)"""
        n = len(hps)
        raw = np.frombuffer(bytes(hps), np.float32)
        if self.hp_pinned is None or self.hp_pinned.numel() < raw.size:
            self.hp_pinned = torch.empty(raw.size, dtype=torch.float32, pin_memory=True)
            self.hp_dev = torch.empty(raw.size, dtype=torch.float32, device=self.device)
            self.hp_event = None
        if self.hp_event is not None:
            self.hp_event.synchronize()
        self.hp_pinned[:raw.size].numpy()[:] = raw
        self.hp_dev[:raw.size].copy_(self.hp_pinned[:raw.size], non_blocking=True)
        self.hp_event = torch.cuda.Event()
        self.hp_event.record()
        assert n * 8 == raw.size
        return self.hp_dev.data_ptr()


def _check(t, what):
    if not isinstance(t, torch.Tensor):
        raise IsfError(f"{what}: expected a tensor, got {type(t).__name__}")
    if t.is_sparse or t.layout != torch.strided:
        raise IsfError(f"{what}: sparse tensors are not supported by the fused optimizer")
    if not t.is_cuda:
        raise IsfError(f"{what}: the fused optimizer runs on the GPU only (HIP kernels); got a CPU tensor. "
                       "There is deliberately no CPU fallback.")
    if t.dtype != torch.float32:
        raise IsfError(f"{what}: the fused optimizer takes float32 tensors, got {t.dtype}")
    if not t.is_contiguous():
        raise IsfError(f"{what}: the fused optimizer takes contiguous tensors")


def _validate(pairs):
    """pairs: [(p, g, state or None)] -> raises IsfError; all on one device"""
    dev = None
    for p, g, st in pairs:
        for t, what in ((p, "parameter"), (g, "gradient")) + (((st["exp_avg"], "exp_avg"),
                                                               (st["exp_avg_sq"], "exp_avg_sq")) if st else ()):
            if t is None:
                continue
            _check(t, what)
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise IsfError(f"{what}: tensors on {dev} and {t.device}; one optimizer step runs on one device")
        if g is not None and p is not None and g.numel() != p.numel():
            raise IsfError(f"gradient of {g.numel()} elements for a parameter of {p.numel()}")
    return dev


def _launch(plan, hps, max_norm, mode):
    lib = _lib.load()
    tab, chk = plan.pointers() if plan.table is not None else (None, None)
    s = _lib.stream()
    clip = mode != _lib.OPTIM_NO_CLIP
    if clip and plan.num_chunks:
        _lib.check(lib.isf_optim_grad_sumsq(tab, chk, plan.num_chunks, plan.partials.data_ptr(), s),
                   "isf_optim_grad_sumsq")
    if not hps:
        hps = (_lib.AdamWHp * 1)()
    hp_dev = plan.hp_device(hps) if len(hps) > _lib.OPTIM_MAX_HP_ARGS else None
    _lib.check(lib.isf_optim_adamw(tab, chk, plan.num_chunks, hps, len(hps), hp_dev,
                                   plan.partials.data_ptr() if clip else None, float(max_norm or 0.0),
                                   plan.norm.data_ptr() if clip else None, mode, s), "isf_optim_adamw")


def _clip_args(grad_clip):
    cfg = dict(grad_clip)
    max_norm = float(cfg.pop("max_norm"))
    norm_type = float(cfg.pop("norm_type", 2))
    cfg.pop("error_if_nonfinite", None)
    if norm_type != 2.0:
        raise NotImplementedError(f"fused gradient clipping supports norm_type=2 only, got {norm_type}")
    if cfg:
        raise NotImplementedError(f"unsupported grad_clip keys {sorted(cfg)}")
    return max_norm


# ------------------------------------------------------------------------------------------------ optimizer
class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (torch 2.x semantics: decoupled weight decay, bias-corrected step) with an optional global-norm
    gradient clip fused in front of it: `step(grad_clip=dict(max_norm=..., norm_type=2))` is mmcv's OptimizerHook
    (clip_grad_norm_ over every gradient, then the optimizer step) in two kernel launches and no host sync.  The
    clipped gradient is used for the update only; `.grad` is left as it is.  `last_grad_norm` is the device scalar of
    the norm (before clipping) of the last clipped step; the next step overwrites it (clone it to keep it).

    Each group's `lr`, `betas`, `eps` and `weight_decay` are read at every step, so torch LR schedulers and the cyclic
    updaters below apply.  State is torch's: `step` a 0-dim float32 CPU tensor, `exp_avg` / `exp_avg_sq` parameter-shaped
    -- state_dict() / load_state_dict() interchange with torch.optim.AdamW both ways."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 maximize=False, foreach=None, capturable=False, differentiable=False, fused=None):
        if amsgrad or maximize or capturable or differentiable:
            raise NotImplementedError("FusedAdamW: amsgrad, maximize, capturable and differentiable are not supported")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=foreach, capturable=False, differentiable=False, fused=fused,
                        decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self._plan = None
        self.last_grad_norm = None

    def __setstate__(self, state):
        super().__setstate__(state)
        for g in self.param_groups:
            for k, v in (("amsgrad", False), ("maximize", False), ("foreach", None), ("capturable", False),
                         ("differentiable", False), ("fused", None), ("decoupled_weight_decay", True)):
                g.setdefault(k, v)
            if g["amsgrad"] or g["maximize"] or g["capturable"] or g["differentiable"]:
                raise NotImplementedError("FusedAdamW: amsgrad, maximize, capturable and differentiable are not "
                                          "supported")

    @torch.no_grad()
    def step(self, closure=None, grad_clip=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        max_norm = _clip_args(grad_clip) if grad_clip is not None else None
        state = self.state
        params, grads, sts, steps, cfgs = [], [], [], [], []
        for group in self.param_groups:
            b1, b2 = group["betas"]
            cfg = (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]))
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                st = state[p]
                if not st:
                    _validate([(p, g, None)])
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                params.append(p)
                grads.append(g)
                sts.append(st)
                steps.append(st["step"])
                cfgs.append(cfg)
        if not params:
            if max_norm is not None:
                self.last_grad_norm = torch.zeros(())
            return loss
        # hyperparameter tuples: one per distinct (group settings, step count), numbered in order of first use
        tvals = torch.stack(steps).tolist() if len(steps) > 1 else [float(steps[0])]
        index, hps, entries = {}, [], []
        for p, g, st, cfg, t in zip(params, grads, sts, cfgs, tvals):
            t += 1.0                                 # the step counter after this step (advanced below, on success)
            k = cfg + (t,)
            i = index.get(k)
            if i is None:
                i = index[k] = len(index)
                lr, b1, b2, eps, wd = cfg
                hps.append((1.0 - lr * wd, 1.0 - b1, b2, 1.0 - b2, eps, -lr / (1.0 - b1 ** t),
                            math.sqrt(1.0 - b2 ** t), 0.0))
            entries.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                            p.numel(), i))
        key = tuple(entries)
        plan = self._plan
        if plan is None or key != plan.key:
            dev = _validate(list(zip(params, grads, sts)))
            if plan is None or plan.device != dev:
                plan = self._plan = _Plan(dev)
            plan.update(key, entries)
        hp_arr = (_lib.AdamWHp * len(hps))(*[_lib.AdamWHp(*h) for h in hps])
        _launch(plan, hp_arr, max_norm, _lib.OPTIM_NO_CLIP if max_norm is None else _lib.OPTIM_CLIP)
        torch._foreach_add_(steps, 1)
        if max_norm is not None:
            self.last_grad_norm = plan.norm
        # the packed-weight caches of the modules see weight changes through Tensor._version only
        torch.autograd.graph.increment_version(params)
        return loss


_CLIP_PLANS = {}


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2):
    """torch.nn.utils.clip_grad_norm_ (norm_type 2): the total L2 norm of every gradient, then g *= min(1, max_norm /
    (norm + 1e-6)) in place -- two launches, no host sync.  Returns the device norm (a scalar the next call with the same
    gradients overwrites)."""
    _clip_args(dict(max_norm=max_norm, norm_type=norm_type))
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    try:
        entries = [(0, g.data_ptr(), 0, 0, g.numel(), 0) for g in grads]
    except RuntimeError:                             # no strided storage (sparse): _validate says why
        entries = None
    key = tuple(entries) if entries is not None else None
    plan = _CLIP_PLANS.get(key)
    if plan is None:
        dev = _validate([(None, g, None) for g in grads])
        if len(_CLIP_PLANS) >= 8:
            _CLIP_PLANS.clear()
        plan = _CLIP_PLANS[key] = _Plan(dev)
        plan.update(key, entries)
    _launch(plan, None, max_norm, _lib.OPTIM_SCALE_GRADS)
    return plan.norm


# ------------------------------------------------------------------------------------------------ mmcv constructor
_PARAMWISE_KEYS = {"custom_keys", "bias_lr_mult", "bias_decay_mult"}
_NORMS = (nn.modules.batchnorm._BatchNorm, nn.modules.instancenorm._InstanceNorm, nn.GroupNorm, nn.LayerNorm)


def build_optimizer(model, cfg):
    """mmcv 1.4 build_optimizer / DefaultOptimizerConstructor for the config's `optimizer` dict (type AdamW only) ->
    FusedAdamW.  With `paramwise_cfg`: one group per parameter in named_parameters() order (frozen ones included, as
    mmcv does); `custom_keys` match as substrings of the dotted name, longest key first (ties alphabetical) and set
    lr = lr * lr_mult, weight_decay = weight_decay * decay_mult; otherwise bias_lr_mult / bias_decay_mult apply to the
    biases of non-norm modules.  Without it: one group of every parameter."""
    cfg = dict(cfg)
    typ = cfg.pop("type", None)
    if typ != "AdamW":
        raise NotImplementedError(f"optimizer type {typ!r}: only AdamW is fused here")
    paramwise = cfg.pop("paramwise_cfg", None)
    if hasattr(model, "module"):
        model = model.module
    if paramwise is None:
        return FusedAdamW(model.parameters(), **cfg)
    unknown = set(paramwise) - _PARAMWISE_KEYS
    if unknown:
        raise NotImplementedError(f"paramwise_cfg keys {sorted(unknown)} are not supported")
    base_lr = cfg.get("lr", 1e-3)
    base_wd = cfg.get("weight_decay", None)
    custom = paramwise.get("custom_keys", {})
    keys = sorted(sorted(custom), key=len, reverse=True)
    bias_lr_mult = paramwise.get("bias_lr_mult", 1.0)
    bias_decay_mult = paramwise.get("bias_decay_mult", 1.0)
    groups = []

    def add(module, prefix):
        is_norm = isinstance(module, _NORMS)
        for name, param in module.named_parameters(recurse=False):
            group = {"params": [param]}
            if not param.requires_grad:
                groups.append(group)
                continue
            full = f"{prefix}.{name}"
            for key in keys:
                if key in full:
                    group["lr"] = base_lr * custom[key].get("lr_mult", 1.0)
                    if base_wd is not None:
                        group["weight_decay"] = base_wd * custom[key].get("decay_mult", 1.0)
                    break
            else:
                if name == "bias" and not is_norm:
                    group["lr"] = base_lr * bias_lr_mult
                    if base_wd is not None:
                        group["weight_decay"] = base_wd * bias_decay_mult
            groups.append(group)
        for child_name, child in module.named_children():
            add(child, f"{prefix}.{child_name}" if prefix else child_name)

    add(model, "")
    return FusedAdamW(groups, **cfg)


# ------------------------------------------------------------------------------------------------ cyclic schedules
def _annealing_cos(start, end, factor):
    return end + 0.5 * (start - end) * (math.cos(math.pi * factor) + 1)


def _annealing_linear(start, end, factor):
    return start + (end - start) * factor


class _Cyclic:
    name = ""

    def __init__(self, config, max_iters):
        cfg = dict(config)
        policy = cfg.pop("policy", None)
        if policy != "cyclic":
            raise NotImplementedError(f"{self.name}_config policy {policy!r}: only 'cyclic' is implemented")
        if cfg.pop("by_epoch", False):
            raise NotImplementedError("cyclic schedules with by_epoch=True")
        if cfg.pop("gamma", 1) != 1:
            raise NotImplementedError("cyclic schedules with gamma != 1")
        ratio = cfg.pop("target_ratio", self.default_ratio)
        if isinstance(ratio, (int, float)):
            ratio = (ratio, ratio / 1e5)
        elif len(ratio) == 1:
            ratio = (ratio[0], ratio[0] / 1e5)
        self.target_ratio = (float(ratio[0]), float(ratio[1]))
        self.cyclic_times = int(cfg.pop("cyclic_times", 1))
        self.step_ratio_up = float(cfg.pop("step_ratio_up", 0.4))
        anneal = cfg.pop("anneal_strategy", "cos")
        if anneal not in ("cos", "linear"):
            raise ValueError(f"anneal_strategy {anneal!r}")
        self.anneal = _annealing_cos if anneal == "cos" else _annealing_linear
        if cfg:
            raise NotImplementedError(f"{self.name}_config keys {sorted(cfg)} are not supported")
        self.max_iters = int(max_iters)
        self.period = self.max_iters // self.cyclic_times
        if self.period < 1:
            raise ValueError(f"max_iters {max_iters} is shorter than cyclic_times {self.cyclic_times}")
        self.up = int(self.step_ratio_up * self.period)

    def value(self, base, it):
        """the scheduled value at iteration `it` for a group whose initial value is `base`"""
        i = it % self.period
        r0, r1 = self.target_ratio
        if i < self.up:
            return self.anneal(base, base * r0, i / self.up)
        return self.anneal(base * r0, base * r1, (i - self.up) / (self.period - self.up))


class CyclicLrUpdater(_Cyclic):
    """mmcv CyclicLrUpdaterHook (by_epoch=False): before iteration `it` every group's lr = value(initial_lr, it)."""
    name, default_ratio = "lr", (10, 1e-4)

    def before_train_iter(self, optimizer, it):
        for g in optimizer.param_groups:
            g.setdefault("initial_lr", g["lr"])
            g["lr"] = self.value(g["initial_lr"], it)


class CyclicMomentumUpdater(_Cyclic):
    """mmcv CyclicMomentumUpdaterHook: every group's momentum -- betas[0] for Adam-type optimizers -- =
    value(initial_momentum, it)."""
    name, default_ratio = "momentum", (0.85 / 0.95, 1)

    def before_train_iter(self, optimizer, it):
        for g in optimizer.param_groups:
            if "initial_momentum" not in g:
                g["initial_momentum"] = g["momentum"] if "momentum" in g else g["betas"][0]
            m = self.value(g["initial_momentum"], it)
            if "momentum" in g:
                g["momentum"] = m
            else:
                g["betas"] = (m, g["betas"][1])


def _updater(cls, cfg, max_iters):
    return None if cfg is None else cls(cfg, max_iters)


class TrainingRecipe:
    """The reference's optimisation of one iteration (mmcv runner order): LR and momentum hooks' before_train_iter,
    then OptimizerHook.after_train_iter's clip + step -- here one fused FusedAdamW step."""

    def __init__(self, optimizer, lr_updater=None, momentum_updater=None, grad_clip=None):
        self.optimizer = optimizer
        self.lr_updater = lr_updater
        self.momentum_updater = momentum_updater
        self.grad_clip = grad_clip

    @classmethod
    def from_config(cls, config, model, max_iters):
        """config: the path of an (unmodified) mmcv-style config file, or the dict of its variables (needs `optimizer`;
        reads `optimizer_config`, `lr_config`, `momentum_config`)."""
        if isinstance(config, str):
            from .registry import load_config
            config = load_config(config)
        if config.get("fp16") is not None:
            raise NotImplementedError("fp16 loss scaling is not part of the fused recipe")
        oc = dict(config.get("optimizer_config") or {})
        if oc.pop("type", "OptimizerHook") != "OptimizerHook":
            raise NotImplementedError("only mmcv's OptimizerHook is mirrored")
        grad_clip = oc.pop("grad_clip", None)
        oc.pop("detect_anomalous_params", None)
        if oc:
            raise NotImplementedError(f"optimizer_config keys {sorted(oc)} are not supported")
        if grad_clip is not None:
            _clip_args(grad_clip)
        return cls(build_optimizer(model, config["optimizer"]),
                   _updater(CyclicLrUpdater, config.get("lr_config"), max_iters),
                   _updater(CyclicMomentumUpdater, config.get("momentum_config"), max_iters), grad_clip)

    def step(self, it):
        """apply the schedules for iteration `it`, then one fused (clip +) AdamW step; -> the device grad norm (None
        without clipping)"""
        if self.lr_updater is not None:
            self.lr_updater.before_train_iter(self.optimizer, it)
        if self.momentum_updater is not None:
            self.momentum_updater.before_train_iter(self.optimizer, it)
        self.optimizer.step(grad_clip=self.grad_clip)
        return self.optimizer.last_grad_norm if self.grad_clip is not None else None
