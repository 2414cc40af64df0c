"""Camera neck: the reference's GeneralizedLSSFPN (mmdet3d/models/necks/generalized_lss.py) on HIP kernels.
Inference only (eval mode).

Top-down step i (from the coarsest level down):  F.interpolate(lateral[i+1], bilinear, align_corners=True) ->
torch.cat([lateral[i], .], 1) -> 1x1 ConvModule (conv, BN, ReLU) is ONE isf_swin_gemm launch whose loader reads the
fine map and interpolates the coarse one on the fly (UPCAT mode); the 3x3 ConvModule runs on the dense-grid f16x3
convolution of dense_conv.py.  State-dict keys: lateral_convs.i.conv / .bn, fpn_convs.i.conv / .bn, as mmcv's
ConvModule names them.
"""
import torch
from torch import nn

from . import _lib
from .dense_conv import PackedConvBN, SplitMap
from .fusion_ops import ACT_NONE, ACT_RELU, PackedLinear, _cache
from .norm import fold_bn
from .swin import _a, _training_error, gemm


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
