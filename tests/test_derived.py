"""derived.py: the one policy behind everything that is derived from module weights (pure Python, CPU tensors,
stand-in values: no library call)."""
import gc

import pytest
import torch
from torch import nn

from isfusion_amd import derived

CPU = torch.device("cpu")


def _tree():
    return nn.Sequential(nn.Linear(4, 4), nn.Sequential(nn.Linear(4, 4), nn.BatchNorm1d(4))).eval()


def _write_in_place(net, leaf):
    with torch.no_grad():
        leaf.weight.mul_(2.0)


def _load_on_ancestor(net, leaf):
    net.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})


def _replace_parameter(net, leaf):
    leaf.weight = nn.Parameter(leaf.weight.detach().clone())


CHANGES = [_write_in_place, _load_on_ancestor, _replace_parameter]


@pytest.mark.parametrize("change", CHANGES)
def test_module_store_follows_the_parameters(change):
    net = _tree()
    leaf = net[1][0]
    for owner, source in ((leaf, None), (net[1], None), (net, leaf), (net, [leaf.weight, leaf.bias])):
        s = derived.store(owner, CPU, source)
        s["packed"] = "stale"
        assert derived.store(owner, CPU, source) is s and derived.store(owner, CPU, source)["packed"] == "stale"
        change(net, leaf)
        s2 = derived.store(owner, CPU, source if not isinstance(source, list) else [leaf.weight, leaf.bias])
        assert s2 is not s and s2 == {}
    # keyed on a sub-module: changes elsewhere below the owner do not count
    s = derived.store(net, CPU, leaf)
    s["packed"] = "kept"
    with torch.no_grad():
        net[0].weight.mul_(2.0)
    assert derived.store(net, CPU, leaf) is s


def test_module_store_is_per_device():
    net = _tree()
    s = derived.store(net, CPU)
    s["packed"] = "cpu"
    other = derived.store(net, torch.device("meta"))        # the same tensors asked for on another device: addresses repeat
    assert other is not s and other == {}
    assert derived.store(net, CPU) == {}


@pytest.mark.parametrize("change", CHANGES)
def test_param_store_follows_the_parameter(change):
    net = _tree()
    leaf = net[1][0]
    s = derived.param_store(leaf.weight)
    s["pair"] = "stale"
    assert derived.param_store(leaf.weight) is s
    change(net, leaf)
    s2 = derived.param_store(leaf.weight)
    assert s2 is not s and s2 == {}


def test_param_store_is_per_device_and_dies_with_its_parameter():
    w = nn.Parameter(torch.zeros(4, 4))
    derived.param_store(w)["pair"] = "cpu"
    hit = derived._by_param[id(w)]
    derived._by_param[id(w)] = (hit[0], (torch.device("meta"), hit[1][1]), hit[2])    # as if packed on another device
    assert derived.param_store(w) == {}
    derived.param_store(w)["pair"] = "old"
    i = id(w)
    del w
    gc.collect()
    assert i not in derived._by_param                                  # the entry went with the parameter
    for _ in range(64):          # new tensors, some of which land on the dead one's id / address (version 0 again)
        v = nn.Parameter(torch.zeros(4, 4))
        assert derived.param_store(v) == {}
        derived.param_store(v)["pair"] = "new"
        del v
    # the guard itself: an entry whose parameter is gone is a miss even when id, device and key agree
    v = nn.Parameter(torch.zeros(4, 4))
    derived.param_store(v)["pair"] = "v"
    dead = nn.Parameter(torch.zeros(1))
    ref = derived._by_param[id(v)][0].__class__(dead)
    del dead
    derived._by_param[id(v)] = (ref, derived._by_param[id(v)][1], {"pair": "a dead tensor's"})
    assert derived.param_store(v) == {}


def test_frozen_owner_is_not_scanned(monkeypatch):
    net = _tree()
    leaf = net[1][0]
    derived.freeze(net)
    assert all(derived.frozen(m) for m in net.modules())
    stores = [derived.store(leaf, CPU), derived.store(net, CPU, leaf)]      # frozen, no store yet: scanned once
    for s in stores:
        s["packed"] = "after the freeze"

    def boom(_):
        raise AssertionError("a frozen owner was scanned")
    monkeypatch.setattr(derived, "param_key", boom)
    assert derived.store(leaf, CPU) is stores[0] and derived.store(net, CPU, leaf) is stores[1]
    for end in (lambda: derived.freeze(net, False), lambda: net.train(), lambda: net[1].load_state_dict(net[1].state_dict())):
        monkeypatch.undo()
        derived.freeze(net.eval())
        derived.store(leaf, CPU)["packed"] = derived.store(net, CPU, leaf)["packed"] = "after the freeze"
        monkeypatch.setattr(derived, "param_key", boom)
        derived.store(leaf, CPU), derived.store(net, CPU, leaf)
        end()
        for owner, source in ((leaf, None), (net, leaf)):
            with pytest.raises(AssertionError, match="scanned"):
                derived.store(owner, CPU, source)
    monkeypatch.undo()
    assert not derived.frozen(net.eval()) and not derived.frozen(leaf)


def test_drop_over_a_mixed_tree():
    net = _tree()
    leaf = net[1][0]
    outside = nn.Linear(4, 4)
    net.__dict__["_graphs"] = {("k",): "captured"}
    derived.store(leaf, CPU)["packed"] = "own"
    derived.store(net, CPU, leaf)["vfe"] = "keyed on a sub-module"
    derived.param_store(leaf.weight)["pair"] = "below"
    derived.param_store(outside.weight)["pair"] = "outside"
    held = nn.Linear(4, 4).eval()                       # driven by the tree without being a registered child
    derived.also_below(net[1], held)
    derived.store(held, CPU)["packed"] = "held"
    derived.param_store(held.weight)["pair"] = "held"
    derived.drop(net)
    assert derived.store(leaf, CPU) == {} and derived.store(net, CPU, leaf) == {} and derived.store(held, CPU) == {}
    assert derived.param_store(leaf.weight) == {} and derived.param_store(held.weight) == {}
    assert net._graphs == {}
    assert derived.param_store(outside.weight) == {"pair": "outside"}
    derived.drop_all()
    assert derived.param_store(outside.weight) == {}
    derived.freeze(net)
    assert derived.frozen(held) and "held" not in list(net.state_dict())
    held.load_state_dict(held.state_dict())      # a load below ends the freeze from the root
    assert not derived.frozen(net)


def test_param_store_switched_off():
    w = nn.Parameter(torch.zeros(4, 4))
    derived.param_store(w)["pair"] = "cached"
    s = derived.param_store(w, enabled=False)
    assert s == {}
    s["pair"] = "not kept"
    assert derived.param_store(w, enabled=False) == {} and id(w) not in derived._by_param
    assert derived.param_store(w) == {}          # and what was cached before the switch is gone


def test_the_names_callers_know():
    from isfusion_amd import fusion_ops as ops, spconv
    assert ops.freeze is derived.freeze and ops.frozen is derived.frozen and ops.drop_caches is derived.drop
    assert ops.param_key is derived.param_key and ops._cache is derived.store
    assert spconv.drop_packed_pairs is derived.drop_all and spconv.PACKED_PAIR_CACHE is True


def test_the_lidar_branch_outside_the_module_tree_is_reached():
    """ISFusionPtsPath keeps its LidarBranch out of the state dict; freeze(), the load hook, train() and drop_caches()
    reach the branch's own store (the VFE fold) all the same"""
    import pickle
    from isfusion_amd import fusion_ops as ops
    from isfusion_amd.detector import ISFusionPtsPath
    net = ISFusionPtsPath().eval()
    lidar = net._lidar.eval()
    assert not any(k.startswith("_lidar") for k in net.state_dict())
    vfe = lidar.pts_voxel_encoder
    derived.store(lidar, CPU, vfe)["vfe"] = "fold"
    ops.drop_caches(net)
    assert derived.store(lidar, CPU, vfe) == {}
    assert net.freeze() is net and derived.frozen(lidar) and derived.frozen(net.pts_middle_encoder)
    derived.store(lidar, CPU, vfe)["vfe"] = "fold"
    net.pts_voxel_encoder.load_state_dict(vfe.state_dict())          # a load below the path: the branch thaws with it
    assert not derived.frozen(lidar) and not derived.frozen(net) and derived.store(lidar, CPU, vfe) == {}
    net.freeze()
    derived.store(lidar, CPU, vfe)["vfe"] = "fold"
    net.train()
    assert not derived.frozen(lidar.eval()) and derived.store(lidar, CPU, vfe) == {}
    assert lidar.freeze() is lidar and derived.frozen(lidar) and not derived.frozen(net.eval())   # on its own, too
    pickle.dumps(net)
