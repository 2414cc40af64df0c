"""CPU tests of the channel-attention backward (A14 training): the C entry isf_channel_attention_backward is exported,
bound and validates its arguments before any HIP call (so none of these calls needs a GPU), and the torch composition
`fusion_train.channel_attention_backward_reference` -- the float32 yardstick of the GPU tests and the Function's other
backward -- is, in float64, the gradient torch.autograd derives from out = a + softmax(a b^T) b."""
import ctypes
import os

import pytest
import torch

ISF_OK, ISF_ERR_ARG, ISF_ERR_UNSUPPORTED = 0, -1, -4


def test_c_entry_is_exported_and_validates_before_any_hip_call():
    from isfusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert "isf_channel_attention_backward" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["isf_channel_attention_backward"][1]) == 8
    lib = _lib.load()
    fn = lib.isf_channel_attention_backward          # AttributeError without the entry
    # pointers that are never dereferenced: every call below returns from the argument checks
    buf = (ctypes.c_float * 4)()
    p = ctypes.addressof(buf)
    for size in (182, 196):
        assert fn(p, p, p, 1, size, p, p, None) == ISF_ERR_UNSUPPORTED
        msg = lib.isf_last_error().decode()
        assert "channel_attention_backward" in msg and str(size) in msg and "192" in msg
    assert fn(p, p, p, 0, 180, p, p, None) == ISF_OK
    assert fn(None, None, None, 0, 180, None, None, None) == ISF_OK        # no maps: nothing is looked at
    assert fn(p, p, p, -1, 180, p, p, None) == ISF_ERR_ARG
    assert fn(p, p, p, 1, -4, p, p, None) == ISF_ERR_ARG
    assert fn(p, p, p, 1, 0, p, p, None) == ISF_ERR_ARG
    # the documented order: both outputs NULL is "nothing to do" even before the inputs and the size are looked at
    assert fn(None, None, None, 3, 182, None, None, None) == ISF_OK
    assert fn(None, p, p, 3, 180, p, None, None) == ISF_ERR_ARG            # null input
    assert fn(None, p, p, 3, 182, p, None, None) == ISF_ERR_ARG            # ... is reported before the unsupported size


@pytest.mark.parametrize("scale", [0.25, 1.0])
@pytest.mark.parametrize("size", [4, 20, 180])
def test_reference_composition_is_the_float64_autograd_gradient(size, scale):
    from isfusion_amd import fusion_train as tr
    gen = torch.Generator().manual_seed(1000 + size)
    maps = 2
    a = (torch.randn((maps, size, size), generator=gen, dtype=torch.float64) * scale).requires_grad_()
    b = (torch.randn((maps, size, size), generator=gen, dtype=torch.float64) * scale).requires_grad_()
    g = torch.randn((maps, size, size), generator=gen, dtype=torch.float64)
    out = a + torch.softmax(a @ b.transpose(1, 2), -1) @ b
    out.backward(g)
    ga, gb = tr.channel_attention_backward_reference(a.detach(), b.detach(), g)
    assert ga.dtype == torch.float64 and ga.shape == a.shape and gb.shape == b.shape
    for got, exact in ((ga, a.grad), (gb, b.grad)):
        assert (got - exact).abs().max().item() <= 1e-12 * exact.abs().max().item()
    # leading dimensions are free: [B, C, H, H] as the Function passes them
    ga4, gb4 = tr.channel_attention_backward_reference(a.detach().view(1, maps, size, size),
                                                       b.detach().view(1, maps, size, size), g.view(1, maps, size, size))
    assert ga4.shape == (1, maps, size, size) and torch.equal(ga4.view_as(ga), ga) and torch.equal(gb4.view_as(gb), gb)
