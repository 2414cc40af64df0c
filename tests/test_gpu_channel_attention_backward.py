"""GPU tests of isf_channel_attention_backward (A14 training; isf_channel_attn_bwd.hip) on its own: parity with the exact
gradient over the kernels' geometry, memory extents, NULL outputs, map independence, repeatability, confinement of
non-finite values, and the route through ChannelAttentionFunction.

The yardstick is never the kernel: `exact` is fusion_train.channel_attention_backward_reference in float64 on the CPU
(tests/test_channel_attention_backward.py pins it to torch.autograd), and the bound is a multiple of the error the SAME
composition makes in float32 on the GPU on the same inputs -- the backward the Function ran before the kernels existed:
    max|kernel - exact| / max|exact|  <=  max(8 * e32, 2e-6)        for gA and gB separately.
8: a different summation order and the fast exponential; 2e-6: cases where the float32 composition happens to be nearly
exact.  Every figure is printed before it is asserted (pytest -s shows them; DESIGN.md section 6 quotes them)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

GEOMETRY = [(1, 4),      # one partial tile
            (3, 20),     # a partial second row tile
            (3, 64),     # exactly one round of the four waves
            (3, 68),     # one row tile into the second round
            (3, 180),    # the path's size
            (2, 192),    # no padding
            (300, 20)]   # more workgroups than CUs


@functools.lru_cache(maxsize=None)
def case(num_maps, size, s, gs):
    """seeded inputs (float32, CPU) and the exact gradients (float64, CPU); computed once, never modified"""
    from isfusion_amd import fusion_train as tr
    gen = torch.Generator().manual_seed(7 * num_maps + size)
    a = torch.randn((num_maps, size, size), generator=gen) * s
    b = torch.randn((num_maps, size, size), generator=gen) * s
    g = torch.randn((num_maps, size, size), generator=gen) * gs
    ga, gb = tr.channel_attention_backward_reference(a.double(), b.double(), g.double())
    return a, b, g, ga, gb


def rel(got, exact):
    return (got.detach().cpu().double() - exact).abs().max().item() / exact.abs().max().item()


def kernel(a, b, g, need_scene=True, need_ins=True):
    """the op on [num_maps, size, size] tensors"""
    from isfusion_amd import fusion_ops as ops
    ga, gb = ops.channel_attention_backward(a[None], b[None], g[None], need_scene, need_ins)
    return (None if ga is None else ga[0]), (None if gb is None else gb[0])


def assert_within_bound(label, got, ref32, exact):
    for name, k, r, e in zip(("gA", "gB"), got, ref32, exact):
        if k is None:
            continue
        ek, e32 = rel(k, e), rel(r, e)
        print(f"{label} {name}: kernel {ek:.3e}  float32 composition {e32:.3e}  ratio {ek / max(e32, 1e-30):.2f}")
        assert torch.isfinite(k).all()
        assert ek <= max(8 * e32, 2e-6), (label, name, ek, e32)


@pytest.mark.parametrize("gs", [1.0, 1e-6])
@pytest.mark.parametrize("s", [0.25, 1.0])
@pytest.mark.parametrize("num_maps,size", GEOMETRY)
def test_parity_over_the_geometry(dev, num_maps, size, s, gs):
    from isfusion_amd import fusion_train as tr
    a, b, g, ga, gb = case(num_maps, size, s, gs)
    ad, bd, gd = a.to(dev), b.to(dev), g.to(dev)
    got = kernel(ad, bd, gd)
    ref32 = tr.channel_attention_backward_reference(ad, bd, gd)
    assert_within_bound(f"maps {num_maps} size {size} s {s} gs {gs}", got, ref32, (ga, gb))


@pytest.mark.parametrize("size", [20, 180])
def test_extents_with_nan_guard_bands(dev, size):
    """the five tensors sit inside larger buffers between NaN guard bands; outputs pre-filled with NaN"""
    from isfusion_amd import _lib
    num_maps, guard = 3, 1024          # guard: a multiple of 4 floats (the tensors stay 16-byte aligned)
    a, b, g, _, _ = case(num_maps, size, 0.25, 1.0)
    n = num_maps * size * size
    bufs = [torch.full((n + 2 * guard,), float("nan"), device=dev) for _ in range(5)]
    for buf, t in zip(bufs, (a, b, g)):
        buf[guard:guard + n] = t.to(dev).reshape(-1)
    before = [buf.clone() for buf in bufs[:3]]
    views = [buf[guard:guard + n] for buf in bufs]
    rc = _lib.load().isf_channel_attention_backward(*[v.data_ptr() for v in views[:3]], num_maps, size,
                                                    views[3].data_ptr(), views[4].data_ptr(), _lib.stream())
    _lib.check(rc, "isf_channel_attention_backward")
    torch.cuda.synchronize()
    for buf in bufs:
        assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + n:]).all()     # guards untouched
    for buf, was in zip(bufs[:3], before):
        assert torch.equal(buf[guard:guard + n], was[guard:guard + n])                   # inputs unchanged
    for out in views[3:]:
        assert torch.isfinite(out).all()           # every element written, and nothing computed from a guard
    ga, gb = kernel(a.to(dev), b.to(dev), g.to(dev))
    assert torch.equal(views[3].view_as(ga), ga) and torch.equal(views[4].view_as(gb), gb)


def test_null_outputs_leave_the_other_output_bit_identical(dev):
    a, b, g, _, _ = [t.to(dev) for t in case(3, 68, 1.0, 1.0)]
    ga, gb = kernel(a, b, g)
    ga_only, none_b = kernel(a, b, g, need_ins=False)
    none_a, gb_only = kernel(a, b, g, need_scene=False)
    assert none_a is None and none_b is None
    assert torch.equal(ga_only, ga) and torch.equal(gb_only, gb)


def test_map_independence_and_repeatability(dev):
    a, b, g, _, _ = [t.to(dev) for t in case(300, 20, 1.0, 1.0)]
    ga, gb = kernel(a, b, g)
    ga2, gb2 = kernel(a, b, g)
    assert torch.equal(ga, ga2) and torch.equal(gb, gb2)                 # the same call twice
    m = 137
    ga1, gb1 = kernel(a[m:m + 1].clone(), b[m:m + 1].clone(), g[m:m + 1].clone())
    assert torch.equal(ga1[0], ga[m]) and torch.equal(gb1[0], gb[m])     # alone = among the 300


def test_nan_in_one_map_stays_in_that_map(dev):
    a, b, g, _, _ = [t.to(dev) for t in case(3, 20, 0.25, 1.0)]
    ga, gb = kernel(a, b, g)
    bad = g.clone()
    bad[1, 7, 9] = float("nan")
    ga_n, gb_n = kernel(a, b, bad)
    for clean, dirty in ((ga, ga_n), (gb, gb_n)):
        assert torch.equal(dirty[0], clean[0]) and torch.equal(dirty[2], clean[2])
        assert not torch.isfinite(dirty[1]).all()


def test_through_autograd(dev, monkeypatch):
    """ChannelAttentionFunction: both inputs, then one input only (needs_input_grad), and autocast"""
    from isfusion_amd import fusion_ops as ops
    from isfusion_amd import fusion_train as tr
    needs = []
    real = ops.channel_attention_backward

    def recording(qs, qi, go, need_scene=True, need_ins=True):
        needs.append((bool(need_scene), bool(need_ins)))
        return real(qs, qi, go, need_scene, need_ins)

    monkeypatch.setattr(ops, "channel_attention_backward", recording)
    a, b, g, _, _ = case(3, 20, 0.25, 1.0)
    a4, b4, g4 = a[None], b[None], g[None]                               # [1, 3, 20, 20]
    ad, bd = a4.double().requires_grad_(), b4.double().requires_grad_()
    (ad + torch.softmax(ad @ bd.transpose(2, 3), -1) @ bd).backward(g4.double())
    exact = (ad.grad[0], bd.grad[0])
    ref32 = tr.channel_attention_backward_reference(a.to(dev), b.to(dev), g.to(dev))
    for want_a, want_b in ((True, True), (True, False), (False, True)):
        x, y = a4.to(dev).requires_grad_(want_a), b4.to(dev).requires_grad_(want_b)
        tr.ChannelAttentionFunction.apply(x, y).backward(g4.to(dev))
        assert needs[-1] == (want_a, want_b)
        assert (x.grad is not None) == want_a and (y.grad is not None) == want_b
        got = (x.grad[0] if want_a else None, y.grad[0] if want_b else None)
        assert_within_bound(f"autograd scene {want_a} ins {want_b}", got, ref32, exact)
    for dtype in (torch.float32, torch.bfloat16):
        x, y = a4.to(dev, dtype).requires_grad_(), b4.to(dev, dtype).requires_grad_()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = tr.ChannelAttentionFunction.apply(x, y)
        out.backward(g4.to(dev, out.dtype))
        for t in (x, y):
            assert t.grad.dtype == dtype and t.grad.shape == t.shape and torch.isfinite(t.grad).all()
    assert len(needs) == 5
