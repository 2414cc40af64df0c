"""GPU tests (-m gpu) of the derived-weight stores (derived.py) at the sites that use them: after every route by which
weights change, a module that has cached packed copies computes what a freshly built module with the new weights
computes -- bit for bit, the kernels and the inputs are the same.  The shapes are the smallest the kernels accept: what is
under test is host bookkeeping."""
import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

FACTOR = 1.25      # a power-of-two-free factor: every packed copy of a scaled weight differs from the stale one


# ------------------------------------------------------------------------------------------------------ sites
class Site:
    """build() -> a module on the device (same seeded weights every time); run(module) -> tuple of tensors;
    packs(module) -> the packed copies it holds after a run (tensors or the objects that own them)."""
    function = False        # True: the site caches per parameter (an autograd Function), not per module


class Lidar(Site):
    # the three-stage middle encoder of test_gpu_widened.test_baseline_config0_hard_vfe_three_stage_encoder behind the
    # DynamicVFE (64 channels): the plan, both conv packings and the VFE fold
    ME = dict(in_channels=64, sparse_shape=[41, 1440, 1440], output_channels=32,
              encoder_channels=((16,), (32,), (64,)), encoder_paddings=((1,), (1,), (1,)))

    def __init__(self, dev):
        from isfusion_amd import synthetic
        self.pts = [torch.from_numpy(np.ascontiguousarray(synthetic.lidar_sweeps(2020, 2000))).to(dev)]
        self.dev = dev

    def build(self):
        import isfusion_amd as m
        return m.LidarBranch(pts_middle_encoder=self.ME).randomize_weights_(3).randomize_bn_(4).eval().to(self.dev)

    def run(self, lb):
        return (lb(self.pts),)

    def packs(self, lb):
        from isfusion_amd.spconv import SparseConvolution
        convs = [c for c in lb.modules() if isinstance(c, SparseConvolution)]
        return ([t for t in lb.pts_middle_encoder._c_plan()[2] if t is not None] + list(lb._vfe_params()[1]) +
                [c.packed_weight() for c in convs] + [c.packed16_weight() for c in convs if c.packed16_weight() is not None])


class Second(Site):
    def __init__(self, dev):
        self.x = torch.randn((2, 128, 36, 36), generator=torch.Generator().manual_seed(5)).mul(0.5).to(dev)
        self.dev = dev

    def build(self):
        from fusion_common import BACKBONE_KW, BB_SEED
        from isfusion_amd.fusion_modules import SECONDV2, seeded_state_dict
        bb = SECONDV2(**BACKBONE_KW).eval()
        bb.load_state_dict(seeded_state_dict(bb, BB_SEED))
        return bb.to(self.dev)

    def run(self, bb):
        with torch.no_grad():
            return tuple(bb(self.x))

    def packs(self, bb):
        return [bb._packed(seq) for seq in (bb.blocks[0], bb.ds_layer, bb.blocks[1])]


class SecondFpn(Site):
    def __init__(self, dev):
        g = torch.Generator().manual_seed(6)
        self.x = [torch.randn((2, 128, 36, 36), generator=g).mul(0.5).to(dev),
                  torch.randn((2, 256, 18, 18), generator=g).mul(0.5).to(dev)]
        self.dev = dev

    def build(self):
        from isfusion_amd.fusion_modules import SECONDFPN, seeded_state_dict
        neck = SECONDFPN().eval()
        neck.load_state_dict(seeded_state_dict(neck, 250))
        return neck.to(self.dev)

    def run(self, neck):
        return tuple(neck(self.x)) + tuple(m.data for m in neck.forward_split(self.x))

    def packs(self, neck):
        from isfusion_amd import fusion_ops as ops
        c = ops._cache(neck, self.dev)
        assert len(c) == 4          # two packed linears, two folded levels
        return [v for k, v in sorted(c.items(), key=lambda kv: str(kv[0]))]


class SparseFunction(Site):
    function = True

    def __init__(self, dev):
        g = torch.Generator().manual_seed(7)
        cells = torch.randperm(8 * 16 * 16, generator=g)[:500].sort().values
        self.idx = torch.stack([torch.zeros_like(cells), cells // 256, cells // 16 % 16, cells % 16], 1).int().to(dev)
        self.feats = torch.randn((500, 32), generator=g).to(dev)
        self.gout = torch.randn((500, 32), generator=g).to(dev)
        self.dev = dev

    def build(self):
        from isfusion_amd.spconv import SubMConv3d
        torch.manual_seed(8)
        return SubMConv3d(32, 32, 3, padding=1).to(self.dev).train()

    def run(self, conv):
        from isfusion_amd.spconv import SparseConvTensor
        x = self.feats.clone().requires_grad_()
        y = conv(SparseConvTensor(x, self.idx, [8, 16, 16], 1)).features
        dx, = torch.autograd.grad(y, x, self.gout)
        return y.detach(), dx

    def packs(self, conv):
        from isfusion_amd import spconv
        w = conv.weight
        return list(spconv._packed_pair(w, w.detach().float().contiguous(), 27, 32, 32))


class DenseFunction(Site):
    function = True

    def __init__(self, dev):
        g = torch.Generator().manual_seed(9)
        self.x = torch.randn((1, 32, 16, 16), generator=g).to(dev)
        self.gout = torch.randn((1, 32, 16, 16), generator=g).to(dev)
        self.dev = dev

    def build(self):
        torch.manual_seed(10)
        return nn.Conv2d(32, 32, 3, padding=1).to(self.dev).train()

    def run(self, conv):
        from isfusion_amd import dense_train
        assert dense_train.usable(conv), "the conv must run on the HIP kernels"
        x = self.x.clone().requires_grad_()
        y = dense_train.conv_stack(conv, x)
        dx, = torch.autograd.grad(y, x, self.gout)
        return y.detach(), dx

    def packs(self, conv):
        from isfusion_amd import dense_train
        return [t for grp in dense_train._groups(conv.weight, False) for t in grp[2:]]


SITES = dict(lidar=Lidar, second=Second, secondfpn=SecondFpn, sparse_function=SparseFunction,
             dense_function=DenseFunction)


@pytest.fixture(scope="module")
def sites(dev):
    made = {}

    def get(name):
        if name not in made:
            made[name] = SITES[name](dev)
        return made[name]
    return get


# ------------------------------------------------------------------------------------------------------ routes
def _in_place(root):
    with torch.no_grad():
        for p in root.parameters():
            p.mul_(FACTOR)


def _load_state_dict(root):
    scaled = {k for k, _ in root.named_parameters()}
    root.load_state_dict({k: v * FACTOR if k in scaled else v.clone() for k, v in root.state_dict().items()})


def _data(root):
    for p in root.parameters():
        p.data.mul_(FACTOR)


def _data_then_drop_caches(root):
    from isfusion_amd import fusion_ops as ops
    _data(root)
    ops.drop_caches(root)


def _data_then_drop_packed_pairs(root):
    from isfusion_amd import spconv
    _data(root)
    spconv.drop_packed_pairs()


ROUTES = dict(in_place=_in_place, load_state_dict=_load_state_dict, data_drop_caches=_data_then_drop_caches,
              data_drop_packed_pairs=_data_then_drop_packed_pairs)
CASES = [(s, r) for s in SITES for r in ROUTES if r != "data_drop_packed_pairs" or SITES[s].function]


def _same(a, b):
    assert len(a) == len(b)
    for t, u in zip(a, b):
        assert t.shape == u.shape and torch.equal(t, u)


@pytest.mark.parametrize("site,route", CASES, ids=[f"{s}-{r}" for s, r in CASES])
def test_weight_change_reaches_the_packed_copies(sites, site, route):
    """fill the caches, change the weights by `route`, run again: bit-equal to a fresh module with the new weights that has
    never cached anything (and the first run is bit-equal to a fresh module's, which makes that comparison meaningful)"""
    s = sites(site)
    root = s.build()
    before = s.run(root)
    _same(before, s.run(s.build()))
    ROUTES[route](root)
    after = s.run(root)
    fresh = s.build()
    fresh.load_state_dict(root.state_dict())
    _same(after, s.run(fresh))
    assert not any(torch.equal(t, u) for t, u in zip(after, before)), "the weight change must show in the outputs"


@pytest.mark.parametrize("site", list(SITES))
def test_unchanged_weights_keep_their_packs(sites, site):
    """packed once per parameter version: with unchanged weights a second call finds the same packed tensors"""
    s = sites(site)
    root = s.build()
    s.run(root)
    first = s.packs(root)
    s.run(root)
    second = s.packs(root)
    assert len(first) == len(second) > 0 and all(a is b for a, b in zip(first, second))


@pytest.mark.parametrize("site", [n for n in SITES if SITES[n].function])
def test_packed_pair_cache_switched_off(sites, site, monkeypatch):
    """spconv.PACKED_PAIR_CACHE = False: the sparse-conv and the dense-conv Function pack on every call, same results"""
    from isfusion_amd import derived, spconv
    s = sites(site)
    root = s.build()
    cached = s.run(root)
    monkeypatch.setattr(spconv, "PACKED_PAIR_CACHE", False)
    _same(cached, s.run(root))
    first, second = s.packs(root), s.packs(root)
    assert len(first) == len(second) > 0 and not any(a is b for a, b in zip(first, second))
    assert id(root.weight) not in derived._by_param


def test_a_frozen_path_is_not_scanned(dev, monkeypatch):
    """the host cost freeze() exists to remove: the second forward of a frozen ISFusionPtsPath asks for no parameter key,
    an unfrozen one does"""
    from detector_common import build_path, detector_inputs
    from isfusion_amd import derived
    calls = []
    key = derived.param_key
    monkeypatch.setattr(derived, "param_key", lambda source: (calls.append(1), key(source))[1])
    net = build_path().to(dev)
    pts, inp, kw, metas = detector_inputs()
    pts = [torch.from_numpy(p).to(dev) for p in pts]
    img_feats = tuple(torch.from_numpy(a).to(dev) for a in inp["img_feats"])

    def scans():
        del calls[:]
        out = net.forward_pts(pts, img_feats, metas, **kw)[0][0]
        return len(calls), {k: out[k].clone() for k in ("center", "height", "dim", "rot", "vel", "heatmap", "dense_heatmap")}
    net.freeze()
    scans()
    n, frozen_out = scans()
    assert n == 0
    net.freeze(False)
    scans()
    n, out = scans()
    assert n > 0
    for k in frozen_out:
        assert torch.equal(frozen_out[k], out[k])
