"""Camera neck: the reference's GeneralizedLSSFPN (mmdet3d/models/necks/generalized_lss.py) on HIP kernels.
``forward`` is the eval-mode forward, ``forward_train`` the training-mode forward with a backward (below).

Top-down step i (from the coarsest level down):  F.interpolate(lateral[i+1], bilinear, align_corners=True) ->
torch.cat([lateral[i], .], 1) -> 1x1 ConvModule (conv, BN, ReLU) is ONE isf_swin_gemm launch whose loader reads the
fine map and interpolates the coarse one on the fly (UPCAT mode); the 3x3 ConvModule runs on the dense-grid f16x3
convolution of dense_conv.py.  State-dict keys: lateral_convs.i.conv / .bn, fpn_convs.i.conv / .bn, as mmcv's
ConvModule names them.

Training (forward_train): the same UPCAT launch without a folded scale / shift gives the raw 1x1 conv rows, BatchNorm with
batch statistics + ReLU is norm.bn1d_relu on the token rows, the 3x3 conv is dense_train.DenseConvFunction.  The 1x1
step's backward (LateralFunction) needs no bilinear sampling in a GEMM: upsampling is linear, so with gradient rows G
    dW[:, :C1] = G^T fine,   dW[:, C1:] = (up^T G)^T coarse,   dcoarse = (up^T G) W[:, C1:]
where up^T (isf_upsample_rows_adjoint) is applied once to the gradient rows; the two dW products run on
isf_rows_weight_grad with the NCHW maps as they are, dcoarse on isf_swin_gemm.
"""
import torch
from torch import nn

from . import _lib
from .dense_conv import PackedConvBN, SplitMap, grid_rulebook
from .fusion_ops import ACT_NONE, ACT_RELU, PackedLinear, _cache
from .norm import fold_bn
from .swin import _a, _training_error, gemm

_amp_fwd = torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
_amp_bwd = torch.amp.custom_bwd(device_type="cuda")


def upsample_rows_adjoint(g, B, H, W, H2, W2):
    """isf_upsample_rows_adjoint: gradient rows g [B*H*W, N] of a map that was F.interpolate(coarse, (H, W), bilinear,
    align_corners=True) -> gradient rows [B*H2*W2, N] of the coarse map"""
    _lib.require_cuda(g)
    assert g.dtype == torch.float32 and g.is_contiguous() and g.shape[0] == B * H * W
    g2 = torch.empty((B * H2 * W2, g.shape[1]), dtype=torch.float32, device=g.device)
    _lib.check(_lib.load().isf_upsample_rows_adjoint(_lib.ptr(g), B, H, W, g.shape[1], H2, W2, _lib.ptr(g2),
                                                     _lib.stream()), "isf_upsample_rows_adjoint")
    return g2


def rows_weight_grad(g, x, inv_scale=None, out=None):
    """isf_rows_weight_grad: dW [N, K] = inv_scale * g^T x for gradient rows g [R, N] and x token rows [R, K] or an NCHW
    map [B, K, H, W] with B*H*W == R.  inv_scale: device scalar (g was pre-scaled by its inverse, _lib.grad_rescale) or
    None.  out: a [N, K] view (row stride >= K, unit column stride) to write into, e.g. a column block of a wider dW."""
    _lib.require_cuda(g, x)
    assert g.dtype == torch.float32 and x.dtype == torch.float32 and g.is_contiguous() and x.is_contiguous()
    R, N = g.shape
    if x.dim() == 4:
        K, hw, ldx = x.shape[1], x.shape[2] * x.shape[3], 0
        assert x.shape[0] * hw == R, (tuple(x.shape), R)
    else:
        assert x.dim() == 2 and x.shape[0] == R
        K, hw, ldx = x.shape[1], 0, x.shape[1]
    if out is None:
        out = torch.empty((N, K), dtype=torch.float32, device=g.device)
    assert tuple(out.shape) == (N, K) and out.stride(1) == 1 and out.dtype == torch.float32
    lib = _lib.load()
    chunks = lib.isf_rows_weight_grad_chunks(R, N, K)
    ws = torch.empty((chunks, N, K), dtype=torch.float32, device=g.device)
    _lib.check(lib.isf_rows_weight_grad(_lib.ptr(g), _lib.ptr(x), ldx, hw, R, N, K, _lib.ptr(inv_scale), _lib.ptr(ws),
                                        chunks, _lib.ptr(out), out.stride(0), _lib.stream()), "isf_rows_weight_grad")
    return out


class LateralFunction(torch.autograd.Function):
    """rows [B*H*W, N] = conv1x1(cat([fine, interpolate(coarse, fine's size, bilinear, align_corners=True)], 1)) without
    a bias, for NCHW maps fine [B, C1, H, W] and coarse [B, C2, H2, W2], weight [N, C1 + C2, 1, 1].  fine gets a
    gradient (G W[:, :C1], NCHW) only when it requires one: forward_train(input_grads=True) on a backbone with a
    backward."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, fine, coarse, weight):
        _lib.require_cuda(fine, coarse, weight)
        fine, coarse = fine.detach().float().contiguous(), coarse.detach().float().contiguous()
        B, C1, H, W = fine.shape
        _, C2, H2, W2 = coarse.shape
        w = weight.detach().float().flatten(1).contiguous()
        ctx.save_for_backward(fine, coarse, w)
        ctx.wshape = tuple(weight.shape)
        return gemm(_a(_lib.SWIN_A_UPCAT, fine, n=B, c=C1, h=H, w=W, x2=coarse, c2=C2, h2=H2, w2=W2), B * H * W, C1 + C2,
                    PackedLinear(w))

    @staticmethod
    @_amp_bwd
    def backward(ctx, grad_rows):
        fine, coarse, w = ctx.saved_tensors
        B, C1, H, W = fine.shape
        _, C2, H2, W2 = coarse.shape
        need_fine, need_coarse, need_w = ctx.needs_input_grad
        if not (need_fine or need_coarse or need_w):
            return None, None, None
        # gradients are tiny: a power-of-two scale keeps the GEMMs' f16 halves in range (exact; up^T is linear)
        gs, sc = _lib.grad_rescale(grad_rows)
        g2 = upsample_rows_adjoint(gs, B, H, W, H2, W2)
        grad_fine = grad_coarse = grad_w = None
        if need_fine:
            # dfine = G W[:, :C1], stored as NCHW by the GEMM's epilogue
            pl = PackedLinear(w[:, :C1].contiguous(), transposed=True)
            grad_fine = gemm(_a(_lib.SWIN_A_ROWS, gs, ldx=gs.shape[1]), gs.shape[0], gs.shape[1], pl,
                             scale=sc[1:].expand(C1).contiguous(), out_nchw=(B, H, W))
        if need_w:
            grad_w = torch.empty((w.shape[0], C1 + C2), dtype=torch.float32, device=w.device)
            rows_weight_grad(gs, fine, sc[1:], out=grad_w[:, :C1])
            rows_weight_grad(g2, coarse, sc[1:], out=grad_w[:, C1:])
            grad_w = grad_w.view(ctx.wshape)
        if need_coarse:
            pl = PackedLinear(w[:, C1:].contiguous(), transposed=True)          # dcoarse = G2 W[:, C1:]
            # (the inverse power-of-two scale rides in the GEMM epilogue's per-column scale: no pass over the rows)
            rows = gemm(_a(_lib.SWIN_A_ROWS, g2, ldx=g2.shape[1]), g2.shape[0], g2.shape[1], pl,
                        scale=sc[1:].expand(C2).contiguous())
            grad_coarse = rows.view(B, H2, W2, C2).permute(0, 3, 1, 2)          # NCHW view of rows, as the forward hands out
        return grad_fine, grad_coarse, grad_w


class ConvModule(nn.Module):
    """mmcv.cnn.ConvModule(conv_cfg=None, norm_cfg=BN2d or None, act_cfg=ReLU or None): conv / bn / activate"""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, norm_cfg=None, act_cfg=None):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, padding=padding, bias=norm_cfg is None)
        if norm_cfg is not None:
            if norm_cfg.get("type") not in ("BN", "BN2d"):
                raise NotImplementedError(f"GeneralizedLSSFPN: norm {norm_cfg} (only BN2d is built)")
            self.bn = nn.BatchNorm2d(out_channels, eps=norm_cfg.get("eps", 1e-5),
                                     momentum=norm_cfg.get("momentum", 0.1))
        else:
            self.bn = None
        if act_cfg is not None:
            if act_cfg.get("type") != "ReLU":
                raise NotImplementedError(f"GeneralizedLSSFPN: activation {act_cfg} (only ReLU is built)")
            self.activate = nn.ReLU(inplace=False)
        else:
            self.activate = None

    def scale_shift(self):
        """(scale, shift) of the folded BN + conv bias, or (None, bias)"""
        b = self.conv.bias.detach().float() if self.conv.bias is not None else None
        if self.bn is None:
            return None, b
        s, t = fold_bn(self.bn)
        if b is not None:
            t = (t + b * s).contiguous()
        return s, t


class GeneralizedLSSFPN(nn.Module):
    """NECKS 'GeneralizedLSSFPN': forward(inputs: list of NCHW maps) -> tuple of num_ins - 1 NCHW maps of out_channels
    (the finer levels after the top-down path)."""

    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, no_norm_on_lateral=False,
                 conv_cfg=None, norm_cfg=dict(type="BN2d"), act_cfg=dict(type="ReLU"),
                 upsample_cfg=dict(mode="bilinear", align_corners=True)):
        super().__init__()
        assert isinstance(in_channels, list)
        if conv_cfg is not None:
            raise NotImplementedError(f"GeneralizedLSSFPN: conv_cfg {conv_cfg} (only Conv2d is built)")
        if start_level != 0 or end_level != -1:
            raise NotImplementedError("GeneralizedLSSFPN: only start_level=0, end_level=-1 are built")
        if dict(upsample_cfg) != dict(mode="bilinear", align_corners=True):
            raise NotImplementedError(f"GeneralizedLSSFPN: upsample {upsample_cfg} (only bilinear, align_corners)")
        if act_cfg is None or norm_cfg is None:
            raise NotImplementedError("GeneralizedLSSFPN: the 3x3 convs need BN2d + ReLU")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.num_ins = len(in_channels)
        self.num_outs = num_outs
        self.no_norm_on_lateral = no_norm_on_lateral
        self.upsample_cfg = dict(upsample_cfg)
        self.backbone_end_level = self.num_ins - 1
        self.start_level = start_level
        self.end_level = end_level
        self.lateral_convs = nn.ModuleList()
        self.fpn_convs = nn.ModuleList()
        for i in range(self.start_level, self.backbone_end_level):
            cin = in_channels[i] + (in_channels[i + 1] if i == self.backbone_end_level - 1 else out_channels)
            self.lateral_convs.append(ConvModule(cin, out_channels, 1, norm_cfg=None if no_norm_on_lateral else norm_cfg,
                                                 act_cfg=act_cfg))
            self.fpn_convs.append(ConvModule(out_channels, out_channels, 3, padding=1, norm_cfg=norm_cfg,
                                             act_cfg=act_cfg))

    def _packed(self, dev):
        c = _cache(self, dev)
        if "lat" not in c:
            with torch.no_grad():
                c["lat"] = []
                for m in self.lateral_convs:
                    s, t = m.scale_shift()
                    c["lat"].append((PackedLinear(m.conv.weight.detach().flatten(1)), s, t, m.activate is not None))
                c["fpn"] = [PackedConvBN(m.conv, m.bn, relu=True) for m in self.fpn_convs]
        return c

    @torch.no_grad()
    def forward(self, inputs):
        if self.training:
            raise _training_error("GeneralizedLSSFPN")
        assert len(inputs) == len(self.in_channels)
        _lib.require_cuda(*inputs)
        lat = [x.float().contiguous() for x in inputs]
        p = self._packed(lat[0].device)
        for i in range(len(lat) - 2, -1, -1):
            fine, coarse = lat[i], lat[i + 1]
            B, C1, H, W = fine.shape
            _, C2, H2, W2 = coarse.shape
            pl, s, t, relu = p["lat"][i]
            y = gemm(_a(_lib.SWIN_A_UPCAT, fine, n=B, c=C1, h=H, w=W, x2=coarse, c2=C2, h2=H2, w2=W2), B * H * W,
                     C1 + C2, pl, scale=s, shift=t, act=ACT_RELU if relu else ACT_NONE, out_nchw=(B, H, W))
            lat[i] = p["fpn"][i](SplitMap.from_nchw(y)).to_nchw()
        return tuple(lat[:len(lat) - 1])

    def forward_train(self, inputs, input_grads=False):
        """Training-mode forward with a backward towards every parameter: batch-statistics BatchNorm (running mean /
        variance and num_batches_tracked move as nn.BatchNorm2d's do), all levels computed as in forward().  inputs: the
        backbone's NCHW maps.  input_grads=False: they come without a gradient (the backbone's default forward_train has
        no backward) and one that requires grad is refused.  input_grads=True: inputs that require grad receive one
        (SwinTransformer.forward_train(..., backward=True)); the parameters' gradients are the same either way.
        Returns NCHW views of token rows."""
        from . import spconv as sp
        from .dense_train import DenseConvFunction, from_rows, supported
        from .norm import bn1d_relu
        assert len(inputs) == len(self.in_channels)
        _lib.require_cuda(*inputs)
        assert self.training, "call .train() first (forward() is the eval-mode forward)"
        if not input_grads and any(x.requires_grad for x in inputs):
            raise NotImplementedError("GeneralizedLSSFPN.forward_train: inputs that require grad need input_grads=True "
                                      "(off by default: the camera backbone's backward is opt-in, and the shipped "
                                      "config detaches its outputs)")
        if self.no_norm_on_lateral:
            raise NotImplementedError("GeneralizedLSSFPN.forward_train: no_norm_on_lateral (biased lateral convs)")
        for m in self.fpn_convs:
            if not supported(m.conv):
                raise NotImplementedError(f"GeneralizedLSSFPN.forward_train: 3x3 conv {m.conv} is outside the dense "
                                          "convolution kernels' channel counts")
        half = bool(sp.AUTOCAST_HALF and torch.is_autocast_enabled())
        lat = list(inputs)
        with torch.autocast("cuda", enabled=False):
            for i in range(len(lat) - 2, -1, -1):
                fine, coarse = lat[i], lat[i + 1]
                B, _, H, W = fine.shape
                lc, fc = self.lateral_convs[i], self.fpn_convs[i]
                rows = LateralFunction.apply(fine, coarse, lc.conv.weight)
                rows = bn1d_relu(lc.bn, rows, relu=lc.activate is not None)
                rows = DenseConvFunction.apply(rows, fc.conv.weight, grid_rulebook(rows.device, B, H, W, 1), False, half)
                rows = bn1d_relu(fc.bn, rows, relu=fc.activate is not None)
                lat[i] = from_rows(rows, B, H, W)
        return tuple(lat[:len(lat) - 1])
