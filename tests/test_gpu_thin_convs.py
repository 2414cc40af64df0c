"""The training path's last library convolutions on the project's kernels (GPU): the thin-K linear pair against float64
with derived bounds, the four sites against the float64 modules with the stock float32 modules on the same GPU as the
yardstick, and two whole training steps: no F.conv* call, and bit-identical repeats without MIOpen's deterministic
attribute."""
import copy
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit round-off of float32


def _rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def rel(got, want, scale=None):
    """max |got - want| / max |want| (or / scale), in float64 on the CPU"""
    want = want.detach().double().cpu()
    return (got.detach().double().cpu() - want).abs().max().item() / (scale or max(want.abs().max().item(), 1e-300))


# ------------------------------------------------------------------------------------------------- thin linear
def _chunk_rows(lib):
    """rows per chunk of the backward's first pass, read off the host query: the largest M that is one chunk"""
    m = 1
    while lib.isf_thin_linear_parts(m + 1) == 1:
        m += 1
    return m


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_thin_linear_against_float64_with_derived_bounds(dev, K):
    """forward, dW, db, dX for M in {1, 63, 65, 400, 4099} x N in {16, 128, 256}, bias present / absent, dX asked for or
    not.  Per element: forward (K + 2) u (sum_k |x w| + |b|) -- K fused multiply-adds behind the bias; dW / db
    (L + 2) u sum_m |g x| with L = rows per chunk + chunks, the longest addition chain of the two fixed-order passes; dX
    (10 + 2) u sum_n |g w| -- four columns in a lane, then the six levels of the xor tree.  Two calls give the same bits."""
    from isfusion_amd import _lib, fusion_train as tr
    lib = _lib.load()
    chunk = _chunk_rows(lib)
    seed = 100 * K
    for M in (1, 63, 65, 400, 4099):
        L = min(M, chunk) + lib.isf_thin_linear_parts(M)
        for N in (16, 128, 256):
            for bias in (True, False):
                for want_dx in (True, False):
                    seed += 1
                    x = _rnd((M, K), seed, 60.0)                 # positions of a 180-cell grid
                    w, b, g = _rnd((N, K), seed + 1000, 0.5), _rnd((N,), seed + 2000), _rnd((M, N), seed + 3000, 1e-3)
                    xd, wd, bd, gd = [t.double() for t in (x, w, b, g)]
                    yr = xd @ wd.t() + (bd if bias else 0.0)
                    y_bound = (K + 2) * U * (xd.abs() @ wd.abs().t() + (bd.abs() if bias else 0.0))
                    runs = []
                    for _ in range(2):
                        xg = x.to(dev).requires_grad_(want_dx)
                        wg, bg = w.to(dev).requires_grad_(), b.to(dev).requires_grad_()
                        y = tr.thin_linear(xg, wg, bg if bias else None)
                        y.backward(g.to(dev))
                        runs.append((y.detach(), wg.grad, bg.grad if bias else None, xg.grad))
                    for a, c in zip(*runs):
                        assert (a is None and c is None) or torch.equal(a, c), (M, N, bias, want_dx)
                    y, gw, gb, gx = [t.double().cpu() if t is not None else None for t in runs[0]]
                    case = (M, K, N, bias, want_dx)
                    assert y.shape == (M, N) and bool(((y - yr).abs() <= y_bound).all()), case
                    assert bool(((gw - gd.t() @ xd).abs() <= (L + 2) * U * (gd.abs().t() @ xd.abs())).all()), case
                    if bias:
                        assert bool(((gb - gd.sum(0)).abs() <= (L + 2) * U * gd.abs().sum(0)).all()), case
                    else:
                        assert gb is None
                    if want_dx:
                        assert bool(((gx - gd @ wd).abs() <= 12 * U * (gd.abs() @ wd.abs())).all()), case
                    else:
                        assert gx is None


def test_thin_linear_refuses_what_it_does_not_tile(dev):
    from isfusion_amd import fusion_train as tr
    from isfusion_amd._lib import IsfError
    for M, K, N in ((10, 9, 128), (10, 2, 24)):
        with pytest.raises(IsfError, match="code -4"):
            tr.thin_linear(torch.zeros((M, K), device=dev), torch.zeros((N, K), device=dev), torch.zeros((N,), device=dev))


# ---------------------------------------------------------------- the sites against the float64 modules
# Bound of an error against float64: twice the error of the stock float32 modules, run on the same GPU, against float64,
# plus the slack tests/test_gpu_train.py allows the same kernels (conv_stack: output 2e-5, input gradient 1e-4, parameter
# gradients 2e-4, buffers 1e-5, output under autocast 2e-2; LinearFunction: output 1e-5, dX 1e-5, dW 1e-4).  Under
# autocast the conv kernels are single-pass f16 and nothing but the 2e-2 is recorded there: it serves every quantity.
SLACK_CONV = dict(out=2e-5, dx=1e-4, dparam=2e-4, buffer=1e-5)
SLACK_LINEAR = dict(out=1e-5, dx=1e-5, dparam=1e-4, buffer=1e-5)
SLACK_AUTOCAST = dict(out=2e-2, dx=2e-2, dparam=2e-2, buffer=2e-2)
REPORT = []


def _check(what, kind, got, stock, want, slack, scale=None):
    e_got, e_stock = rel(got, want, scale), rel(stock, want, scale)
    REPORT.append((what, kind, e_got, e_stock))
    print(f"{what}: {kind}: kernels {e_got:.3e}  stock float32 {e_stock:.3e}  bound {2 * e_stock + slack[kind]:.3e}")
    return e_got <= 2 * e_stock + slack[kind], (what, kind, e_got, e_stock)


def _assert_all(results):
    bad = [info for ok, info in results if not ok]
    assert not bad, bad


def _three_ways(make_ref, run, autocast, dev, monkeypatch, what, slack, inputs):
    """run(module, inputs) -> output on (a) the float64 module on the CPU, (b) the float32 module on the GPU with
    fusion_train.STOCK_CONVS = True (the stock nn.Conv* calls), (c) the same with the kernels; compares output, input
    gradients, parameter gradients and buffers of (c) with (a), bounded by (b)'s"""
    from isfusion_amd import fusion_train as tr
    ref = make_ref().double().train()
    start = copy.deepcopy(ref.state_dict())
    xr = [t.double().requires_grad_() for t in inputs]
    yr = run(ref, xr)
    up = _rnd(tuple(yr.shape), 5)
    (yr * up.double()).sum().backward()
    outs = {}
    for stock in (True, False):
        net = make_ref()
        net.load_state_dict(start)
        net = net.float().to(dev).train()
        xg = [t.to(dev).requires_grad_() for t in inputs]
        monkeypatch.setattr(tr, "STOCK_CONVS", stock)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            y = run(net, xg)
        (y.float() * up.to(dev)).sum().backward()
        outs[stock] = (y, xg, net)
    (y, xg, net), (ys, xs, nets) = outs[False], outs[True]
    assert y.shape == yr.shape
    res = [_check(what, "out", y, ys, yr, slack)]
    for a, s, r in zip(xg, xs, xr):
        res.append(_check(what, "dx", a.grad, s.grad, r.grad, slack))
    pr = dict(ref.named_parameters())
    assert len(pr) > 0
    # a gradient that is ZERO in exact arithmetic -- the bias in front of a batch-statistics BatchNorm, which subtracts the
    # mean again: 1e-26 in float64 -- has no scale of its own; what float32 leaves there is the rounding of a sum of that
    # layer's output gradients, so it is measured against the layer's largest gradient (its weight's, the same sums)
    layer = {}
    for n, q in pr.items():
        k = n.rpartition(".")[0]
        layer[k] = max(layer.get(k, 0.0), q.grad.abs().max().item())
    for (n, p), (_, q) in zip(net.named_parameters(), nets.named_parameters()):
        assert p.grad is not None and p.grad.shape == pr[n].grad.shape, n
        top = layer[n.rpartition(".")[0]]
        scale = top if pr[n].grad.abs().max().item() < 1e-9 * top else None
        res.append(_check(what + " " + n, "dparam", p.grad, q.grad, pr[n].grad, slack, scale))
    br = dict(ref.named_buffers())
    for (n, b), (_, c) in zip(net.named_buffers(), nets.named_buffers()):
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(c) == int(br[n]) == 1, n
        else:
            res.append(_check(what + " " + n, "buffer", b, c, br[n], slack))
    _assert_all(res)


@pytest.mark.parametrize("shape", [(1, 37, 2), (2, 200, 2)], ids=["1x37", "2x200"])
def test_pos_embed_training_matches_the_float64_module(dev, shape, monkeypatch):
    """fusion_ops._pos_embed in training mode (thin-K kernel / fused BatchNorm + ReLU / fused linear kernel) against
    PositionEmbeddingLearned in float64 on the CPU: output, BatchNorm buffers, the six parameter gradients, E = 128"""
    from isfusion_amd import fusion_ops as ops
    from isfusion_amd.fusion_modules import PositionEmbeddingLearned, seeded_state_dict

    def make():
        m = PositionEmbeddingLearned(2, 128)
        m.load_state_dict(seeded_state_dict(m, 41))
        return m

    xy = torch.rand(shape, generator=torch.Generator().manual_seed(9)) * 180.0

    def run(m, xs):
        if xs[0].is_cuda:
            return ops._pos_embed(m, xs[0])
        return m.position_embedding_head(xs[0].transpose(1, 2)).transpose(1, 2)
    _three_ways(make, run, False, dev, monkeypatch, "pos_embed %dx%d" % shape[:2], SLACK_LINEAR, [xy])
    assert len(list(make().parameters())) == 6


@pytest.mark.parametrize("autocast", [False, True], ids=["float32", "autocast_bf16"])
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("cin", [64, 128])
def test_narrow_conv_stack_matches_float64_conv2d(dev, cin, transpose, autocast, monkeypatch):
    """conv_stack(narrow=True) on cin -> 10 with bias (the two heat-map convs), B = 2, 12 x 10, against float64 F.conv2d
    autograd on the plain / permuted map"""
    from isfusion_amd import dense_train as dt, fusion_train as tr

    def make():
        conv = torch.nn.Conv2d(cin, 10, 3, padding=1, bias=True)
        g = torch.Generator().manual_seed(cin)
        conv.weight.data = torch.randn(conv.weight.shape, generator=g) * 0.05
        conv.bias.data = torch.randn(conv.bias.shape, generator=g) * 0.5
        return conv

    x = _rnd((2, cin, 12, 10), 3)

    def run(conv, xs):
        if xs[0].is_cuda:
            if not tr.STOCK_CONVS:
                assert dt.usable(conv, True), "the conv must run on the HIP kernels"
            return dt.conv_stack(conv, xs[0], transpose, narrow=not tr.STOCK_CONVS)
        if transpose:
            return F.conv2d(xs[0].permute(0, 1, 3, 2), conv.weight, conv.bias, padding=1).permute(0, 1, 3, 2)
        return F.conv2d(xs[0], conv.weight, conv.bias, padding=1)
    _three_ways(make, run, autocast, dev, monkeypatch, f"conv {cin}->10 transpose={transpose} autocast={autocast}",
                SLACK_AUTOCAST if autocast else SLACK_CONV, [x])


NECKS = {
    "level0_5x7": (dict(in_channels=(128,), out_channels=(256,), upsample_strides=(1,)), [(2, 128, 5, 7)]),
    "level1_3x4": (dict(in_channels=(256,), out_channels=(256,), upsample_strides=(2,)), [(2, 256, 3, 4)]),
    "both": (dict(), [(2, 128, 6, 8), (2, 256, 3, 4)]),
    "reduced": (dict(in_channels=(32, 64), out_channels=(64, 32)), [(2, 32, 6, 8), (2, 64, 3, 4)]),
}


@pytest.mark.parametrize("autocast", [False, True], ids=["float32", "autocast_bf16"])
@pytest.mark.parametrize("name", list(NECKS))
def test_neck_training_matches_the_float64_modules(dev, name, autocast, monkeypatch):
    """SECONDFPN in train() on the GPU (fused linear kernel + fused BatchNorm) against the float64 modules; the shapes of
    tests/test_thin_convs.py"""
    from isfusion_amd.fusion_modules import SECONDFPN, seeded_state_dict
    kw, shapes = NECKS[name]

    def make():
        neck = SECONDFPN(**kw)
        neck.load_state_dict(seeded_state_dict(neck, 250))
        neck.dense_conv = "hip"
        return neck

    xs = [_rnd(s, 20 + i) for i, s in enumerate(shapes)]

    def run(neck, x):
        if not x[0].is_cuda:
            neck.dense_conv = "stock"
        return neck(x)[0]
    # (under autocast the GEMMs stay fp32-class: LinearFunction's slack in both modes)
    _three_ways(make, run, autocast, dev, monkeypatch, f"neck {name} autocast={autocast}", SLACK_LINEAR, xs)


# ------------------------------------------------------------------------------------------ whole training steps
_PATH = {}


def _T(a):
    return torch.as_tensor(a).to("cuda:0")


def _path():
    if not _PATH:
        from detector_common import build_path, detector_inputs
        from isfusion_amd import head_loss, synthetic
        net = build_path()
        net.pts_bbox_head.train_cfg = dict(head_loss.SHIPPED_TRAIN_CFG)
        net = net.to("cuda:0")
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


def _step(d, net, autocast):
    leaves = [x.detach().clone().requires_grad_(True) for x in d["img"]]
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        ld = net.forward_train(d["pts"], leaves, d["metas"], d["gtb"], d["gtl"], **d["kw"])
        loss = sum(v.float() for k, v in ld.items() if k != "matched_ious")
    loss.backward()
    return ld, leaves


@pytest.mark.parametrize("autocast", [False, True], ids=["float32", "autocast_bf16"])
def test_a_training_step_calls_no_library_convolution(dev, autocast, monkeypatch):
    """one forward_train + backward of the points path with the shipped head config: F.conv1d, F.conv2d and
    F.conv_transpose2d (what every nn.Conv* module calls) are never entered; with fusion_train.STOCK_CONVS = True the
    same counters see the four sites"""
    from isfusion_amd import fusion_train as tr
    calls = {}

    def counted(name):
        inner = getattr(F, name)

        def f(*a, **k):
            calls[name] += 1
            return inner(*a, **k)
        return f
    names = ("conv1d", "conv2d", "conv_transpose2d")
    for n in names:
        monkeypatch.setattr(F, n, counted(n))
    d = _path()
    seen = {}
    with _rng_restored():
        for stock in (False, True):
            monkeypatch.setattr(tr, "STOCK_CONVS", stock)
            calls.update({n: 0 for n in names})
            ld, _ = _step(d, _fresh(d), autocast)
            assert all(bool(torch.isfinite(v).all()) for v in ld.values())
            seen[stock] = dict(calls)
    _fresh(d)
    print("F.conv* calls per step:", seen)
    assert seen[False] == {n: 0 for n in names}, seen
    assert all(seen[True][n] > 0 for n in names), seen


@pytest.mark.parametrize("autocast", [False, True], ids=["float32", "autocast_bf16"])
def test_deterministic_mode_repeats_without_the_library_attribute(dev, autocast):
    """deterministic mode with torch.backends.cudnn.deterministic put back to False inside it: three steps from the same
    state and seeds give the same bits -- every loss, the camera-feature gradient, every parameter gradient.  (With
    stock convolutions in the step their weight gradients differ run to run here.)"""
    import isfusion_amd
    d = _path()
    runs = []
    with _rng_restored(), isfusion_amd.deterministic():
        inside = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = False
        try:
            for _ in range(3):
                net = _fresh(d)
                ld, leaves = _step(d, net, autocast)
                r = {"loss " + k: v.detach().clone() for k, v in ld.items()}
                assert leaves[1].grad is not None and float(leaves[1].grad.abs().max()) > 0
                r["camera feature gradient"] = leaves[1].grad.clone()
                grads = {"grad " + n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
                assert len(grads) > 100
                r.update(grads)
                runs.append(r)
        finally:
            torch.backends.cudnn.deterministic = inside
    _fresh(d)
    for r in runs[1:]:
        assert list(r) == list(runs[0])
    differ = sorted({k for r in runs[1:] for k in r if not torch.equal(r[k], runs[0][k])})
    assert differ == [], differ
