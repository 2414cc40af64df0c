"""Host-side checks of the training path's last convolutions moved onto the project's kernels: the data paths around the
kernels in float64 against the stock nn modules (no GPU), and the C ABI of the thin-K linear pair."""
import copy
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-10


def rel(got, want):
    return (got.detach() - want.detach()).abs().max().item() / max(want.detach().abs().max().item(), 1e-300)


# ---------------------------------------------------------------------------------------------------- SECONDFPN
def _f64_linear(t, w):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) @ w.t()


def _bn_relu(bn, rows):
    from isfusion_amd.norm import bn1d_relu       # on CPU rows: the stock batch_norm composition over the rows
    return bn1d_relu(bn, rows, relu=True)


def _neck_case(neck, shapes, seed):
    """forward_train_tokens with a float64 GEMM against the stock deblocks in train() mode: output, running statistics,
    num_batches_tracked, input gradients, every parameter gradient"""
    from isfusion_amd.fusion_modules import seeded_state_dict
    neck.load_state_dict(seeded_state_dict(neck, seed))
    neck = neck.double().train()
    ref = copy.deepcopy(neck)
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    xa, xb = [x.clone().requires_grad_() for x in xs], [x.clone().requires_grad_() for x in xs]
    want = torch.cat([d(x) for d, x in zip(ref.deblocks, xb)], 1).permute(0, 1, 3, 2)
    got = neck.forward_train_tokens(xa, _f64_linear, _bn_relu)[0]
    assert got.shape == want.shape
    assert rel(got, want) < BOUND
    up = torch.randn(want.shape, generator=g, dtype=torch.float64)
    (got * up).sum().backward()
    (want * up).sum().backward()
    for a, b in zip(xa, xb):
        assert rel(a.grad, b.grad) < BOUND
    pa, pb = dict(neck.named_parameters()), dict(ref.named_parameters())
    assert len(pa) == 3 * len(shapes)
    for n in pa:
        assert pa[n].grad.shape == pb[n].grad.shape and rel(pa[n].grad, pb[n].grad) < BOUND, n
    ba, bb = dict(neck.named_buffers()), dict(ref.named_buffers())
    for n in ba:
        if n.endswith("num_batches_tracked"):
            assert int(ba[n]) == int(bb[n]) == 1, n
        else:
            assert rel(ba[n], bb[n]) < BOUND, n
            assert not torch.equal(ba[n], torch.zeros_like(ba[n])) and not torch.equal(ba[n], torch.ones_like(ba[n])), n


def test_neck_training_data_path_equals_the_stock_deblocks():
    """B = 2, non-square maps (a swapped H / W in the final permute changes the shape and every value).  A 5 x 7 level 0
    and a 3 x 4 level 1 cannot share one concatenated map (3 x 4 up-samples to 6 x 8), so those two shapes run as
    one-level necks and the two-level neck -- channel offsets of the concatenation, six parameter gradients -- runs 6 x 8
    with 3 x 4; then the same on a width-reduced copy."""
    from isfusion_amd.fusion_modules import SECONDFPN
    _neck_case(SECONDFPN(in_channels=(128,), out_channels=(256,), upsample_strides=(1,)), [(2, 128, 5, 7)], 11)
    _neck_case(SECONDFPN(in_channels=(256,), out_channels=(256,), upsample_strides=(2,)), [(2, 256, 3, 4)], 12)
    _neck_case(SECONDFPN(), [(2, 128, 6, 8), (2, 256, 3, 4)], 13)
    _neck_case(SECONDFPN(in_channels=(32, 64), out_channels=(64, 32)), [(2, 32, 6, 8), (2, 64, 3, 4)], 14)


def test_neck_training_weights_are_the_folded_layout_without_the_fold():
    """_train_weights(i) stacked = _folded(i)'s weight when the BatchNorm is the identity (scale 1, shift 0)"""
    from isfusion_amd.fusion_modules import SECONDFPN, seeded_state_dict
    neck = SECONDFPN()
    neck.load_state_dict(seeded_state_dict(neck, 3))
    for d in neck.deblocks:
        d[1].eps = 0.0
        torch.nn.init.ones_(d[1].weight), torch.nn.init.zeros_(d[1].bias)
        torch.nn.init.ones_(d[1].running_var), torch.nn.init.zeros_(d[1].running_mean)
    for i in range(2):
        ws, s = neck._train_weights(i)
        w, _, s2 = neck._folded(i)
        assert s == s2 and torch.equal(torch.cat(list(ws), 0), w)


# ---------------------------------------------------------------------------------------- padded output columns
class _F64Conv:
    """dense_train._HipConv's interface on F.conv2d: the convolution on `cols` zero-padded output columns.  Its weight
    gradient carries a 1 in every padding row, which the caller has to drop."""
    seen = []

    @staticmethod
    def rulebook(device, B, H, W, stride):
        assert stride == 1
        return types.SimpleNamespace(B=B, H=H, W=W, num_out=B * H * W, out_shape=(H, W))

    @staticmethod
    def _conv(rows, wp, rb, transpose):
        x = rows.view(rb.B, rb.H, rb.W, -1).permute(0, 3, 1, 2)
        y = F.conv2d(x.permute(0, 1, 3, 2), wp, padding=1).permute(0, 1, 3, 2) if transpose else F.conv2d(x, wp, padding=1)
        return y.permute(0, 2, 3, 1).reshape(rb.num_out, -1)

    @classmethod
    def forward(cls, rows, weight, cols, rb, transpose, mode):
        wp = F.pad(weight.detach(), (0, 0, 0, 0, 0, 0, 0, cols - weight.shape[0]))
        return cls._conv(rows, wp, rb, transpose), [rows]

    @classmethod
    def backward(cls, saved, weight, cols, grad_out, rb, transpose, mode, want_dx, want_dw):
        cout = weight.shape[0]
        assert grad_out.shape == (rb.num_out, cols) and not grad_out[:, cout:].any()      # zero gradient into the padding
        rows = saved[0].detach().requires_grad_()
        wp = F.pad(weight.detach(), (0, 0, 0, 0, 0, 0, 0, cols - cout)).requires_grad_()
        with torch.enable_grad():
            y = cls._conv(rows, wp, rb, transpose)
        gx, gw = torch.autograd.grad(y, (rows, wp), grad_out)
        gw = gw.clone()
        gw[cout:] = 1.0
        cls.seen.append((cols, tuple(gw.shape)))
        return gx, gw


@pytest.mark.parametrize("transpose", [False, True])
def test_narrow_conv_on_padded_columns_equals_conv2d(transpose):
    """conv_stack(narrow=True) on a 64 -> 10 conv with bias: 32 columns inside, 10 outside; output, input gradient, weight
    and bias gradients against F.conv2d on the plain / permuted map, the padding's weight gradient dropped"""
    from isfusion_amd import dense_train as dt
    g = torch.Generator().manual_seed(7 + transpose)
    conv = torch.nn.Conv2d(64, 10, 3, padding=1, bias=True).double()
    x = torch.randn((2, 64, 6, 5), generator=g, dtype=torch.float64)
    up = torch.randn((2, 10, 6, 5), generator=g, dtype=torch.float64)
    assert dt.padded_columns(10) == 32 and dt.padded_columns(32) == 32 and dt.padded_columns(64) == 64
    assert dt.usable(conv, True, _F64Conv) and not dt.usable(conv, False, _F64Conv)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    if transpose:
        want = F.conv2d(xb.permute(0, 1, 3, 2), conv.weight, conv.bias, padding=1).permute(0, 1, 3, 2)
    else:
        want = F.conv2d(xb, conv.weight, conv.bias, padding=1)
    gw_want, gb_want, gx_want = torch.autograd.grad((want * up).sum(), (conv.weight, conv.bias, xb))
    _F64Conv.seen.clear()
    got = dt.conv_stack(conv, xa, transpose, narrow=True, impl=_F64Conv)
    assert got.shape == want.shape == (2, 10, 6, 5) and rel(got, want) < BOUND
    (got * up).sum().backward()
    assert _F64Conv.seen == [(32, (32, 64, 3, 3))]
    assert conv.weight.grad.shape == (10, 64, 3, 3) and rel(conv.weight.grad, gw_want) < BOUND
    assert rel(conv.bias.grad, gb_want) < BOUND and rel(xa.grad, gx_want) < BOUND
    # not asked for: the module itself
    assert torch.equal(dt.conv_stack(conv, x, False, impl=_F64Conv), conv(x))


# -------------------------------------------------------------------------------------------------------- ABI
NEW_SYMBOLS = ("isf_thin_linear_forward", "isf_thin_linear_parts", "isf_thin_linear_backward")


def test_thin_linear_abi_and_host_query():
    from isfusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(isf_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "fusion_encoder.py:173-189" in open(os.path.join(ROOT, "include", "isf_hip.h")).read()
    parts = [lib.isf_thin_linear_parts(m) for m in (1, 63, 64, 65, 4099, 64800)]
    assert all(p > 0 for p in parts) and parts == sorted(parts) and parts[0] == 1
    assert lib.isf_thin_linear_parts(0) == 0
    # the shape domain is refused before any launch (no GPU here or there)
    unsupported = int(re.search(r"#define ISF_ERR_UNSUPPORTED \((-?\d+)\)", hdr).group(1))
    for n, k in ((128, 9), (24, 2), (128, 0), (272, 2)):
        assert lib.isf_thin_linear_forward(1, 1, None, 1, 5, n, k, None) == unsupported
        assert lib.isf_thin_linear_backward(1, 1, 1, 1, 1, None, None, 5, n, k, None) == unsupported


def test_stock_convs_switch_defaults_to_the_kernels():
    from isfusion_amd import fusion_train
    assert fusion_train.STOCK_CONVS is False
