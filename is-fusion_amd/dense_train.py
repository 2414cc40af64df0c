"""Dense 3x3 BEV convolutions + BatchNorm2d (batch statistics) + ReLU in TRAINING mode on the HIP kernels
(SURVEY.md 8f #2 / #4).

The reference trains these stacks on cuDNN: mmcv ConvModule (fusion_encoder.py:862-960: conv_fusion, conv_ins, conv_scene,
conv_heatmap, heatmap_head_1/2) and SECONDV2 (backbones/second.py:126-165).  Until round 6 the training step ran them on
MIOpen (bf16 igemm + Col2Im2dU + layout transposes + casts: 7.9 ms of a 48-ms step at 2 x 300 k points,
gpurun_out/r06_train).  Here a dense [B, H, W] grid is a sparse tensor with every cell active, as in the inference path
(dense_conv.py):

* forward  = the sparse-conv kernel over the cached arithmetic rulebook of the grid (isf_dense_grid_rulebook),
* dX       = the same kernel over the transposed rulebook with the per-tap transposed filters,
* dW       = isf_sparse_conv_backward_filter_f16x3 (f16 matrix cores) over the rulebook's pair lists,
* BN + ReLU = the fused BatchNorm kernels of norm.py on the [tokens, C] rows (channels-last BatchNorm2d IS BatchNorm1d
  over the token rows), synchronised across ranks for naiveSyncBN2d.

Activations travel through a stack as fp32 token rows ([B*H*W, C], token = (b*H + y)*W + x); a stack hands back an NCHW
*view* of its rows, so the token-major ops around it (SST, attention) pay no layout copy.  Arithmetic: f16x3 split
(fp32-class) by default, single-pass f16 under torch.autocast -- what the reference's autocast does to its convolutions
(bf16 there; f16 operands + fp32 accumulation here, like the sparse convolutions: spconv.AUTOCAST_HALF).

Fewer than 32 output channels (the 10-class heat-map convs of the fusion encoder and the detection head): the same
kernels with the filter zero-padded to their narrowest tile, 32 columns, as the inference path does (dense_conv.py); the
output rows and the weight gradient are sliced back (conv_stack(..., narrow=True); fusion_train.STOCK_CONVS = True keeps
those two on the stock module).

No CPU fallback: layers the kernels do not tile (other channel counts than 32 / 64 / 128 / 256 per <= 256-channel input
group) run on the stock module, everything else fails loudly without the HIP library.
"""
import torch
from torch import nn

from . import _lib, derived
from . import spconv as sp
from .dense_conv import grid_rulebook
from .norm import bn1d_relu

ENABLED = True        # False: every stack on the stock modules (the round-5 training path; A/B and cross-check)

_amp_fwd = torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
_amp_bwd = torch.amp.custom_bwd(device_type="cuda")


MIN_COLUMNS = 32     # the kernels' narrowest output tile: a narrower conv runs with its filter zero-padded to it


def padded_columns(cout):
    """output columns a conv with `cout` output channels runs with (dense_conv.PackedConvBN pads the same way)"""
    return MIN_COLUMNS if cout < MIN_COLUMNS else cout


def _shape_supported(conv, narrow=False):
    if not (isinstance(conv, nn.Conv2d) and conv.kernel_size == (3, 3) and conv.padding == (1, 1) and
            conv.dilation == (1, 1) and conv.groups == 1 and conv.stride in ((1, 1), (2, 2)) and
            conv.padding_mode == "zeros"):
        return False
    cin, cout = conv.in_channels, conv.out_channels
    if narrow:                       # e.g. the 10-class heat-map convs: padded columns
        cout = padded_columns(cout)
    return cout in sp.F16X3_CHANNELS and cin >= 32 and cin % 256 in (0, 32, 64, 128)   # <= 256-channel input groups


def supported(conv, narrow=False):
    """can this nn.Conv2d run on the kernels?  narrow: also with fewer than MIN_COLUMNS output channels (padded columns)"""
    return _shape_supported(conv, narrow) and conv.weight.is_cuda


def _groups(weight, transpose):
    """packed (forward, dX) filters per <= 256-channel input group of a Conv2d weight [Cout, Cin, 3, 3], once per
    parameter version: [(offset, channels, forward filters, dX filters)] (derived.param_store, with the sparse convs'
    switch spconv.PACKED_PAIR_CACHE).  Fewer than MIN_COLUMNS output channels: zero filters up to MIN_COLUMNS -- cached
    on the PARAMETER like every other, not on a padded temporary."""
    s = derived.param_store(weight, sp.PACKED_PAIR_CACHE)
    if ("groups", bool(transpose)) in s:
        return s["groups", bool(transpose)]
    w = weight.detach().float()
    cout, cin = w.shape[:2]
    if padded_columns(cout) != cout:
        w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 0, 0, padded_columns(cout) - cout))
        cout = w.shape[0]
    # taps enumerated (ky, kx); transpose: (kx, ky) = the convolution of the spatially transposed map on the
    # un-transposed tokens (dense_conv.PackedConvBN)
    w5 = (w.permute(3, 2, 1, 0) if transpose else w.permute(2, 3, 1, 0)).contiguous()      # [3, 3, Cin, Cout]
    groups = []
    off = 0
    while off < cin:
        c = min(256, cin - off)
        wk = w5[:, :, off:off + c].contiguous().view(1, 3, 3, c, cout)
        groups.append((off, c, sp.pack_filters_f16x3(wk), *sp.pack_filters_dx(wk)))     # forward | dX filters, their headroom
        off += c
    s["groups", bool(transpose)] = groups
    return groups


class _HipConv:
    """the kernels behind DenseConvFunction, on `cols` = padded_columns(Cout) output columns (tests/test_thin_convs.py
    puts a float64 torch convolution in their place to check the padding algebra around them on the CPU)"""

    @staticmethod
    def rulebook(device, B, H, W, stride):
        return grid_rulebook(device, B, H, W, stride)

    @staticmethod
    def forward(rows, weight, cols, rb, transpose, mode):
        """-> (rows [num_out, cols], tensors to save)"""
        _lib.require_cuda(rows, weight)
        groups = _groups(weight, transpose)
        saved = []
        out = None
        for off, c, pk, _, _ in groups:
            xs = sp.to_split(rows if len(groups) == 1 else rows[:, off:off + c])
            y = sp.from_split(sp.sparse_conv_split(xs, pk, 9, c, cols, rb, ordered=False, mode=mode), (rb.num_out, cols))
            out = y if out is None else out.add_(y)
            saved.append(xs)
        return out, saved

    @staticmethod
    def backward(saved, weight, cols, grad_out, rb, transpose, mode, want_dx, want_dw):
        """grad_out [num_out, cols] -> (grad rows | None, grad weight [cols, Cin, 3, 3] | None)"""
        cin = weight.shape[1]
        groups = _groups(weight, transpose)
        gs, sc = sp.grad_to_split(grad_out)
        grad_rows = grad_w = None
        # (WGRAD_FULL_TAPS: every tap list of a dense grid is full -- larger reduction chunks, a third of the partial-sum traffic)
        parts = [sp.split_backward(xs, gs, sc, rb, pkt, 9, c, cols, bool(mode & _lib.CONV_MODE_F16), want_dx, want_dw,
                                   (1, 3, 3, c, cols), _lib.WGRAD_FULL_TAPS, dx_room=room)
                 for xs, (_, c, _, pkt, room) in zip(saved, groups)]
        if want_dx:
            grad_rows = parts[0][0] if len(parts) == 1 else torch.cat([dx for dx, _ in parts], 1)
        if want_dw:
            g5 = (parts[0][1] if len(parts) == 1 else torch.cat([dw for _, dw in parts], 3)).view(3, 3, cin, cols)
            grad_w = g5.permute(3, 2, 1, 0) if transpose else g5.permute(3, 2, 0, 1)
        return grad_rows, grad_w


class DenseConvFunction(torch.autograd.Function):
    """rows [B*H*W, Cin] fp32, weight [Cout, Cin, 3, 3] -> rows [B*OH*OW, Cout] fp32 (no bias).  Cout < MIN_COLUMNS: the
    kernels run on MIN_COLUMNS columns (zero filters), the output rows and the weight gradient are sliced back to Cout --
    the padding's columns get a zero output gradient and their weight gradient is dropped."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, rows, weight, rb, transpose, half, impl=_HipConv):
        cout = weight.shape[0]
        cols = padded_columns(cout)
        mode = _lib.CONV_MODE_F16 if half else 0
        out, saved = impl.forward(rows.detach(), weight, cols, rb, bool(transpose), mode)
        ctx.save_for_backward(*saved)
        ctx.weight_ref, ctx.version = weight, weight._version
        ctx.geom = (rb, bool(transpose), mode, cout, cols, impl)
        return out if cols == cout else out[:, :cout].contiguous()

    @staticmethod
    @_amp_bwd
    def backward(ctx, grad_out):
        rb, transpose, mode, cout, cols, impl = ctx.geom
        weight = ctx.weight_ref
        assert weight._version == ctx.version, "conv weight modified between forward and backward"
        want_dx, want_dw = ctx.needs_input_grad[:2]
        if cols != cout:
            grad_out = torch.nn.functional.pad(grad_out, (0, cols - cout))
        grad_rows, grad_w = impl.backward(ctx.saved_tensors, weight, cols, grad_out, rb, transpose, mode, want_dx, want_dw)
        if grad_w is not None:
            grad_w = grad_w[:cout].contiguous()
        return grad_rows, grad_w, None, None, None, None


def to_rows(x):
    """[B, C, H, W] (any strides) -> fp32 rows [B*H*W, C]; free when x is the NCHW view of token-major rows"""
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C).float().contiguous()


def from_rows(rows, B, H, W):
    """NCHW VIEW of token-major rows (no copy)"""
    return rows.view(B, H, W, rows.shape[1]).permute(0, 3, 1, 2)


def _layers(seq):
    """nn.Sequential of (Conv2d [, BatchNorm2d] [, ReLU])* -> [(conv, bn | None, relu)] or None"""
    mods = list(seq)
    out = []
    i = 0
    while i < len(mods):
        conv = mods[i]
        if not isinstance(conv, nn.Conv2d):
            return None
        bn = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], nn.modules.batchnorm._BatchNorm) else None
        j = i + (2 if bn is not None else 1)
        relu = j < len(mods) and isinstance(mods[j], nn.ReLU)
        out.append((conv, bn, relu))
        i = j + (1 if relu else 0)
    return out


def usable(seq, narrow=False, impl=_HipConv):
    """does this stack run on the kernels in the current mode?  (narrow: supported())"""
    if not (ENABLED and sp.TRAINING_KERNELS and sp.WGRAD_F16X3 and torch.is_grad_enabled()):
        return False
    ls = _layers(seq if isinstance(seq, nn.Sequential) else nn.Sequential(seq))
    ok = supported if impl is _HipConv else _shape_supported
    return ls is not None and all(ok(c, narrow) for c, _, _ in ls)


def conv_stack(seq, x, transpose=False, narrow=False, impl=_HipConv):
    """training-mode forward of an nn.Sequential of (Conv2d 3x3 [, BatchNorm2d] [, ReLU])* -- a ConvModule, a SECONDV2
    block, a single Conv2d -- on [B, C, H, W] (or a list of such maps = their channel concatenation); returns an NCHW view
    of token-major rows.  Weights written through `.data` need fusion_ops.drop_caches(module) before the next call (the
    packed filters are keyed on Tensor._version).  transpose=True: the stack
    applied to x.permute(0, 1, 3, 2), result permuted back (what the reference does around its instance branch,
    fusion_encoder.py:1093,1139) without transposing anything.  Stacks the kernels do not cover run on the stock modules.
    narrow=True: a conv with fewer than MIN_COLUMNS output channels runs on the kernels too, on zero-padded columns (the
    callers that train the 10-class heat-map convs ask for it; without it such a conv stays on the stock module).
    impl: the kernels (_HipConv), replaceable by a restatement with the same interface."""
    single = not isinstance(seq, nn.Sequential)
    if isinstance(x, (list, tuple)):     # channel concatenation of several maps (conv_fusion's input, fusion_encoder.py:1163)
        if usable(seq, narrow, impl):            # written token-major in one pass per source: to_rows() below is then a view
            x = torch.cat([t.permute(0, 2, 3, 1).float() for t in x], 3).permute(0, 3, 1, 2)
        else:
            x = torch.cat(list(x), 1)
    if not usable(seq, narrow, impl):
        if transpose:
            y = seq(x.permute(0, 1, 3, 2).contiguous())
            return y.permute(0, 1, 3, 2)
        return seq(x)
    layers = _layers(nn.Sequential(seq) if single else seq)
    B, _, H, W = x.shape
    half = bool(sp.AUTOCAST_HALF and torch.is_autocast_enabled())
    with torch.autocast("cuda", enabled=False):
        rows = to_rows(x) if impl is _HipConv else x.permute(0, 2, 3, 1).reshape(B * H * W, -1)
        for conv, bn, relu in layers:
            rb = impl.rulebook(rows.device, B, H, W, conv.stride[0])
            rows = DenseConvFunction.apply(rows, conv.weight, rb, transpose, half, impl)
            H, W = rb.out_shape
            if conv.bias is not None:
                rows = rows + (conv.bias.float() if impl is _HipConv else conv.bias)
            if bn is not None:
                rows = bn1d_relu(bn, rows, relu=relu)
            elif relu:
                rows = torch.relu(rows)
        return from_rows(rows, B, H, W)
