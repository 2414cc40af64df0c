"""Everything derived from module weights -- packed filters and linears, folded BatchNorm, the sparse encoder's C plan,
the VFE parameter block, window tables -- is kept in the stores of this module, under one policy:

* one change detector, param_key(): (Tensor._version, data_ptr) of the tensors, compared together with the device
  (addresses repeat across devices).  Optimizer steps, load_state_dict and every in-place op move it; writes through
  `.data` do NOT -- after such a write call drop(module);
* store(owner, device): a dict owned by a module, replaced by an empty one when the key moved, used without looking at
  the parameters while the owner is frozen;
* param_store(weight): the same for the autograd Functions, which see a weight and no module;
* freeze() / frozen(): one flag per module; every change of it drops what lies below;
* drop(module) / drop_all(): forget.  Captured HIP graphs (`_graphs` dicts) go with the stores: their kernels hold
  pointers into the packed copies.

This module imports nothing from the package, so every other module may use it.
"""
import weakref

from torch import nn

_STORE, _FROZEN, _ROOT, _ALSO = "_isf_derived", "_isf_frozen", "_isf_freeze_root", "_isf_also"

_by_param = {}      # id(parameter) -> (weak reference to it, (device, key), dict)


def param_key(source):
    """(version, address) of every parameter and buffer below a module, or of every tensor of an iterable: changes
    whenever one of them is replaced or written in place -- by load_state_dict (mmcv's load_checkpoint recurses over
    _load_from_state_dict and never fires the post hooks), an optimizer step or a manual copy_()."""
    if isinstance(source, nn.Module):
        source = list(source.parameters()) + list(source.buffers())
    return tuple((t._version, t.data_ptr()) for t in source)


def also_below(module, *others):
    """Modules that `module` drives without registering them as children (ISFusionPtsPath keeps its LidarBranch out of
    the state dict that way) count as lying below it for freeze() and drop()."""
    module.__dict__[_ALSO] = tuple(others)


def _below(module):
    seen = set()
    todo = [module]
    while todo:
        for sub in todo.pop().modules():
            if id(sub) not in seen:
                seen.add(id(sub))
                todo.extend(sub.__dict__.get(_ALSO, ()))
                yield sub


# ------------------------------------------------------------------------------------------------------ stores
def store(owner, device, source=None):
    """The dict of values derived for `owner` on `device`; `source` (a module or a list of tensors, default: the owner)
    is what they were derived from.  A new, empty dict when the device or the key of `source` moved.  A frozen owner
    that has a store uses it without a scan (one with no store yet scans once).
    An owner has ONE store: every caller of an owner passes the same `source`, or they would empty each other's values.
    `device` is a tensor's `.device` (torch.device("cuda") != torch.device("cuda:0") would miss on every call)."""
    hit = owner.__dict__.get(_STORE)
    if hit is not None and hit[0] == device and frozen(owner):
        return hit[2]
    key = param_key(owner if source is None else source)
    if hit is None or hit[0] != device or hit[1] != key:
        hit = owner.__dict__[_STORE] = (device, key, {})
    return hit[2]


def param_store(weight, enabled=True):
    """The dict of values derived from one parameter.  Entries are found by identity and guarded by a weak reference:
    a new tensor that reuses a dead one's id, address and version 0 misses, and an entry goes with its parameter.
    enabled=False (spconv.PACKED_PAIR_CACHE, read by the callers at call time): nothing cached comes back, nothing is
    kept."""
    if not enabled:
        _by_param.pop(id(weight), None)
        return {}
    hit = _by_param.get(id(weight))
    key = (weight.device, param_key((weight,)))
    if hit is None or hit[0]() is not weight or hit[1] != key:
        def forget(ref, i=id(weight)):      # the parameter died: its entry goes, unless the id already serves a new one
            if _by_param.get(i, (None,))[0] is ref:
                del _by_param[i]
        hit = _by_param[id(weight)] = (weakref.ref(weight, forget), key, {})
    return hit[2]


def drop(module):
    """Forget everything that was derived from the parameters below `module`: the stores of its modules and of their
    parameters, and captured HIP graphs."""
    for sub in _below(module):
        d = sub.__dict__
        d.pop(_STORE, None)
        if isinstance(d.get("_graphs"), dict):
            d["_graphs"].clear()
        for p in sub.parameters(recurse=False):
            hit = _by_param.get(id(p))
            if hit is not None and hit[0]() is p:
                del _by_param[id(p)]


def drop_all():
    """Forget every parameter-owned store (module-owned ones are reached through their module: drop())."""
    _by_param.clear()


# ------------------------------------------------------------------------------------------------------ freeze
def _unfreeze_on_load(module, *_):
    """load_state_dict pre-hook (fires inside every module's _load_from_state_dict, so also under mmcv's
    load_checkpoint): new weights are coming, the packed copies must be re-derived."""
    freeze(module.__dict__.get(_ROOT, module), False)


def freeze(module, flag=True):
    """Inference deployments: skip the per-call "did a parameter change?" scan of the stores below `module`.
    The skip ends by itself when weights can change: a load_state_dict anywhere below `module`, or a forward in
    training mode (see frozen()), clears it -- call freeze() again once the weights are final.

    Every change of the flag -- freezing, unfreezing, the load_state_dict hook -- DROPS the derived state below
    `module` (drop): a frozen store is used without looking at the parameters, so it must have been filled after
    the freeze; load_state_dict -> freeze() -> forward, or train() -> optimizer steps -> eval() -> freeze(), would
    otherwise reuse copies packed from the old weights (and replay HIP graphs that point into them)."""
    drop(module)
    for sub in _below(module):
        sub.__dict__[_FROZEN] = bool(flag)
        if flag:
            if _ROOT not in sub.__dict__:
                sub._register_load_state_dict_pre_hook(_unfreeze_on_load, with_module=True)
            sub.__dict__[_ROOT] = module
    return module


def flagged(module):
    """the raw flag: freeze() was called and nothing has ended it yet (no look at the training mode, no side effect)"""
    return module.__dict__.get(_FROZEN, False)


def frozen(module):
    """True when `module`'s store may be used without checking the parameters.  A module seen in training mode loses
    the flag (an optimizer step is about to change its weights; a later eval() then re-validates by key)."""
    if not flagged(module):
        return False
    if module.training:
        module.__dict__[_FROZEN] = False
        return False
    return True
