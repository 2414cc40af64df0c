"""Camera backbone: the reference's SwinTransformer (mmdet3d/models/backbones/swin.py, with PatchEmbed / PatchMerging of
models/utils/transformer.py) on the HIP kernels of isf_swin.hip.  ``forward`` is the eval-mode forward;
``forward_train`` is the training-mode forward (stochastic depth) without a backward: the shipped config detaches the
backbone's outputs (``detach=True``, isfusion.py:76-77), so training needs no gradient through it.

Same sub-module names, parameters and buffers as the reference, so an IS-Fusion checkpoint's ``img_backbone.*`` loads
with ``strict=True`` (187 entries for configs/isfusion/isfusion_0075voxel.py, mmcv FFN naming ``ffn.layers.0.0`` /
``ffn.layers.1``).  Per SwinBlock (token rows [N*H*W, C]):

    row stats -> qkv GEMM (norm1 prologue) -> window attention -> proj GEMM (+ identity)
    row stats -> fc1 GEMM (norm2 prologue, GELU) -> fc2 GEMM (+ identity)

PatchEmbed is one GEMM whose loader gathers the 4 x 4 x 3 patches from the NCHW image (+ a LayerNorm pass), PatchMerging
one GEMM whose loader gathers the 2 x 2 neighbourhood (+ its LayerNorm prologue), the out_indices norms one LayerNorm
pass that stores NCHW.  Packed weights are derived once per parameter version (fusion_ops._cache).

``set_precision("f16")`` switches the eval-mode forward to the f16 inference mode (isf_swin_gemm_f16,
isf_swin_window_attention_f16): one matrix instruction per product instead of three, and the branch intermediates --
qkv [M, 3C], the attention output [M, C], the FFN hidden [M, 4C] -- are f16 rows.  The residual stream, LayerNorm
statistics, softmax, GELU and every accumulation stay fp32, PatchEmbed / PatchMerging write fp32 rows, and the
out_indices maps are the same fp32 NCHW tensors.  Both modes run the one schedule above through ``gemm`` and
``window_attention``: the precision is carried by the packed weight (PackedLinear / PackedLinearF16) and by the dtype of
the qkv rows, nothing else.  Each mode's packed weights live under its name in the same per-module cache.
``precision`` is a plain attribute: no parameter, no buffer, no constructor argument.
"""
import ctypes

import torch
from torch import nn

from . import _lib
from .fusion_ops import ACT_GELU, ACT_NONE, PackedLinear, _cache

WINDOW_TOKENS = 49


def _a(mode, x, *, ldx=0, n=0, c=0, h=0, w=0, x2=None, c2=0, h2=0, w2=0, stats=None, ln=None):
    """isf_swin_a for the loader `mode` (keeps the tensors it points to alive through the returned tuple)"""
    g = b = None
    if ln is not None:
        g, b = ln
    s = _lib.SwinA(_lib.ptr(x), _lib.ptr(x2), _lib.ptr(stats), _lib.ptr(g), _lib.ptr(b), mode, ldx, n, c, h, w, c2, h2,
                   w2)
    return s, (x, x2, stats, g, b)


class PackedLinearF16:
    """nn.Linear weights as one plane of f16 MFMA fragments (isf_pack_linear_f16), for the f16 inference mode"""

    def __init__(self, weight):
        _lib.require_cuda(weight)
        w = weight.detach().float().contiguous()
        self.out_features, self.in_features = w.shape
        lib = _lib.load()
        self.packed = torch.empty(lib.isf_packed_linear_f16_bytes(self.out_features, self.in_features),
                                  dtype=torch.uint8, device=w.device)
        _lib.check(lib.isf_pack_linear_f16(_lib.ptr(w), self.out_features, self.in_features, _lib.ptr(self.packed),
                                           _lib.stream()), "isf_pack_linear_f16")


def gemm(a, rows, k, pl, *, scale=None, shift=None, act=ACT_NONE, residual=None, out_nchw=None, row_scale=None,
         out_f16=False):
    """act((A W^T) * scale + shift) + residual -> [rows, N], or [B, N, H, W] for out_nchw=(B, H, W).  A comes from the
    loader `a`.  The packed weight carries the precision: a PackedLinear goes to isf_swin_gemm (f16x3 products), a
    PackedLinearF16 to isf_swin_gemm_f16 (single-pass products; when the loader's x is an f16 tensor its rows are read
    as they are, and out_f16 stores f16 rows).
    row_scale [samples] (isf_swin_gemm_rowscale): the branch output of sample r // (rows // samples) is multiplied by
    row_scale[sample] before the residual is added (DropPath)."""
    s, keep = a
    N = pl.out_features
    x = keep[0]
    f16 = isinstance(pl, PackedLinearF16)
    if f16 and row_scale is not None:
        raise NotImplementedError("swin.gemm: row_scale with a PackedLinearF16 (isf_swin_gemm_f16 has no row scale)")
    if out_f16 and not f16:
        raise NotImplementedError("swin.gemm: out_f16 with an f16x3 PackedLinear (isf_swin_gemm stores fp32)")
    if out_nchw is not None:
        B, H, W = out_nchw
        shape, ldy, y_hw = (B, N, H, W), 0, H * W
    else:
        shape, ldy, y_hw = (rows, N), N, 0
    y = torch.empty(shape, dtype=torch.float16 if out_f16 else torch.float32, device=x.device)
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.is_contiguous() and tuple(residual.shape) == (rows, N)
    lib = _lib.load()
    # what the three entries share: the operands before y, and y's layout after it
    ops = (rows, k, _lib.ptr(pl.packed), N, _lib.ptr(scale), _lib.ptr(shift), act, _lib.ptr(residual))
    lay = (ldy, y_hw, _lib.stream())
    if f16:
        _lib.check(lib.isf_swin_gemm_f16(ctypes.byref(s), int(x.dtype == torch.float16), *ops, _lib.ptr(y),
                                         int(out_f16), *lay), "isf_swin_gemm_f16")
    elif row_scale is not None:
        assert row_scale.dtype == torch.float32 and row_scale.is_contiguous() and rows % row_scale.numel() == 0
        _lib.check(lib.isf_swin_gemm_rowscale(ctypes.byref(s), *ops, _lib.ptr(row_scale), rows // row_scale.numel(),
                                              _lib.ptr(y), *lay), "isf_swin_gemm_rowscale")
    else:
        _lib.check(lib.isf_swin_gemm(ctypes.byref(s), *ops, _lib.ptr(y), *lay), "isf_swin_gemm")
    return y


def row_stats(a, rows, k, eps):
    """isf_swin_row_stats -> [rows, 2] (mean, rstd)"""
    s, keep = a
    st = torch.empty((rows, 2), dtype=torch.float32, device=keep[0].device)
    _lib.check(_lib.load().isf_swin_row_stats(ctypes.byref(s), rows, k, float(eps), _lib.ptr(st), _lib.stream()),
               "isf_swin_row_stats")
    return st


def layernorm(x, norm, out_nchw=None):
    """isf_swin_layernorm of token rows [M, C] -> rows, or [B, C, H, W] for out_nchw=(B, H, W)"""
    M, C = x.shape
    if out_nchw is not None:
        B, H, W = out_nchw
        y = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
        hw = H * W
    else:
        y = torch.empty_like(x)
        hw = 0
    _lib.check(_lib.load().isf_swin_layernorm(_lib.ptr(x), M, C, _lib.ptr(norm.weight), _lib.ptr(norm.bias),
                                              float(norm.eps), _lib.ptr(y), hw, _lib.stream()), "isf_swin_layernorm")
    return y


def window_attention(qkv, qkv_bias, rel_bias, B, H, W, C, heads, window, shift, scale):
    """qkv rows [B*H*W, 3C] -> attention output rows [B*H*W, C] (before proj) of qkv's dtype: fp32 rows go to
    isf_swin_window_attention, f16 rows to isf_swin_window_attention_f16"""
    entry = {torch.float32: "isf_swin_window_attention", torch.float16: "isf_swin_window_attention_f16"}[qkv.dtype]
    assert qkv.is_contiguous() and tuple(qkv.shape) == (B * H * W, 3 * C)
    out = torch.empty((B * H * W, C), dtype=qkv.dtype, device=qkv.device)
    _lib.check(getattr(_lib.load(), entry)(_lib.ptr(qkv), _lib.ptr(qkv_bias), _lib.ptr(rel_bias), B, H, W, C, heads,
                                           window, shift, float(scale), _lib.ptr(out), _lib.stream()), entry)
    return out


def _ln_only(norm_cfg):
    if (norm_cfg or {}).get("type", "LN") != "LN":
        raise NotImplementedError(f"SwinTransformer: norm {norm_cfg} (only LN is built)")


def _training_error(what):
    return NotImplementedError(f"{what}: forward() is the eval() mode forward; in training mode call forward_train "
                               "(stochastic depth / batch-statistics BatchNorm)")


class WindowMSA(nn.Module):
    """swin.py:20-113 (parameters and the relative_position_index buffer)"""

    def __init__(self, embed_dims, num_heads, window_size, qkv_bias=True, qk_scale=None, attn_drop_rate=0.,
                 proj_drop_rate=0.):
        super().__init__()
        self.embed_dims = embed_dims
        self.window_size = window_size
        self.num_heads = num_heads
        self.scale = qk_scale or (embed_dims // num_heads) ** -0.5
        self.relative_position_bias_table = nn.Parameter(
            torch.zeros((2 * window_size[0] - 1) * (2 * window_size[1] - 1), num_heads))
        Wh, Ww = window_size
        seq = self.double_step_seq(2 * Ww - 1, Wh, 1, Ww)
        self.register_buffer("relative_position_index", (seq + seq.T).flip(1).contiguous())
        self.qkv = nn.Linear(embed_dims, embed_dims * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop_rate)
        self.proj = nn.Linear(embed_dims, embed_dims)
        self.proj_drop = nn.Dropout(proj_drop_rate)

    @staticmethod
    def double_step_seq(step1, len1, step2, len2):
        seq1 = torch.arange(0, step1 * len1, step1)
        seq2 = torch.arange(0, step2 * len2, step2)
        return (seq1[:, None] + seq2[None, :]).reshape(1, -1)

    def relative_bias(self):
        """[heads, 49, 49] = table[index] (swin.py:87-93), gathered on the device"""
        n = self.window_size[0] * self.window_size[1]
        t = self.relative_position_bias_table.detach().float()
        return t[self.relative_position_index.view(-1)].view(n, n, -1).permute(2, 0, 1).contiguous()


class ShiftWindowMSA(nn.Module):
    """swin.py:116-283"""

    def __init__(self, embed_dims, num_heads, window_size, shift_size=0, qkv_bias=True, qk_scale=None,
                 attn_drop_rate=0, proj_drop_rate=0, drop_path_rate=0.):
        super().__init__()
        self.window_size = window_size
        self.shift_size = shift_size
        assert 0 <= shift_size < window_size
        self.w_msa = WindowMSA(embed_dims, num_heads, (window_size, window_size), qkv_bias, qk_scale, attn_drop_rate,
                               proj_drop_rate)
        self.drop_path_rate = drop_path_rate


class FFN(nn.Module):
    """mmcv.cnn.bricks.transformer.FFN with num_fcs=2, add_identity=True: layers = [[Linear, GELU, Dropout], Linear,
    Dropout] (state-dict names layers.0.0 / layers.1)"""

    def __init__(self, embed_dims, feedforward_channels, ffn_drop=0., drop_path_rate=0.):
        super().__init__()
        self.embed_dims = embed_dims
        self.feedforward_channels = feedforward_channels
        self.layers = nn.Sequential(
            nn.Sequential(nn.Linear(embed_dims, feedforward_channels), nn.GELU(), nn.Dropout(ffn_drop)),
            nn.Linear(feedforward_channels, embed_dims), nn.Dropout(ffn_drop))
        self.drop_path_rate = drop_path_rate


class SwinBlock(nn.Module):
    """swin.py:286-368"""

    def __init__(self, embed_dims, num_heads, feedforward_channels, window_size=7, shift=False, qkv_bias=True,
                 qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0., act_cfg=dict(type="GELU"),
                 norm_cfg=dict(type="LN")):
        super().__init__()
        _ln_only(norm_cfg)
        if (act_cfg or {}).get("type") != "GELU":
            raise NotImplementedError(f"SwinBlock: activation {act_cfg} (only GELU is built)")
        self.norm1 = nn.LayerNorm(embed_dims)
        self.attn = ShiftWindowMSA(embed_dims, num_heads, window_size, window_size // 2 if shift else 0, qkv_bias,
                                   qk_scale, attn_drop_rate, drop_rate, drop_path_rate)
        self.norm2 = nn.LayerNorm(embed_dims)
        self.ffn = FFN(embed_dims, feedforward_channels, drop_rate, drop_path_rate)

    def pack(self, linear=PackedLinear):
        """linear: PackedLinear (default mode) or PackedLinearF16 (f16 inference mode)"""
        m = self.attn.w_msa
        l1, l2 = self.ffn.layers[0][0], self.ffn.layers[1]
        return dict(qkv=linear(m.qkv.weight), qkv_b=None if m.qkv.bias is None else m.qkv.bias.detach(),
                    proj=linear(m.proj.weight), proj_b=m.proj.bias.detach(), rel=m.relative_bias(),
                    fc1=linear(l1.weight), fc1_b=l1.bias.detach(), fc2=linear(l2.weight), fc2_b=l2.bias.detach())

    def run(self, p, x, B, H, W, keep=(None, None)):
        """x: token rows [B*H*W, C] -> the block's output rows; x and the result are the fp32 residual rows.  With the
        f16 pack (pack(PackedLinearF16)) qkv, the attention output and the FFN hidden are f16 rows.  keep: per-image
        DropPath factors [B] (keep / keep_prob) of the attention and the FFN branch, or None: the branch output is
        multiplied by them after window reverse / un-shift and before the identity is added (swin.py:251, mmcv FFN);
        gemm refuses them with the f16 pack."""
        M, C = x.shape
        m = self.attn.w_msa
        h16 = isinstance(p["qkv"], PackedLinearF16)
        ln1 = (self.norm1.weight.detach(), self.norm1.bias.detach())
        st = row_stats(_a(_lib.SWIN_A_ROWS, x, ldx=C), M, C, self.norm1.eps)
        qkv = gemm(_a(_lib.SWIN_A_ROWS, x, ldx=C, stats=st, ln=ln1), M, C, p["qkv"], shift=p["qkv_b"], out_f16=h16)
        att = window_attention(qkv, p["qkv_b"], p["rel"], B, H, W, C, m.num_heads, self.attn.window_size,
                               self.attn.shift_size, m.scale)
        x = gemm(_a(_lib.SWIN_A_ROWS, att, ldx=C), M, C, p["proj"], shift=p["proj_b"], residual=x, row_scale=keep[0])
        ln2 = (self.norm2.weight.detach(), self.norm2.bias.detach())
        st = row_stats(_a(_lib.SWIN_A_ROWS, x, ldx=C), M, C, self.norm2.eps)
        F = self.ffn.feedforward_channels
        h = gemm(_a(_lib.SWIN_A_ROWS, x, ldx=C, stats=st, ln=ln2), M, C, p["fc1"], shift=p["fc1_b"], act=ACT_GELU,
                 out_f16=h16)
        return gemm(_a(_lib.SWIN_A_ROWS, h, ldx=F), M, F, p["fc2"], shift=p["fc2_b"], residual=x, row_scale=keep[1])


class PatchEmbed(nn.Module):
    """utils/transformer.py:134-258 with conv_type Conv2d, padding 'corner', kernel = stride"""

    def __init__(self, in_channels=3, embed_dims=96, kernel_size=4, stride=4, norm_cfg=None):
        super().__init__()
        if kernel_size != 4 or stride != 4:
            raise NotImplementedError(f"PatchEmbed: kernel {kernel_size} / stride {stride} (only 4 / 4 is built)")
        self.embed_dims = embed_dims
        self.projection = nn.Conv2d(in_channels, embed_dims, kernel_size, stride)
        if norm_cfg is not None:
            _ln_only(norm_cfg)
            self.norm = nn.LayerNorm(embed_dims)
        else:
            self.norm = None

    def pack(self, linear=PackedLinear):
        """linear: PackedLinear (default mode) or PackedLinearF16 (f16 inference mode)"""
        w = self.projection.weight.detach().float().flatten(1)           # [C, cin*16], k = ci*16 + ky*4 + kx
        k = (w.shape[1] + 31) // 32 * 32
        wp = torch.cat([w, w.new_zeros(w.shape[0], k - w.shape[1])], 1)
        return dict(w=linear(wp), b=self.projection.bias.detach().float().contiguous(), k=k)

    def run(self, p, img):
        N, C, H, W = img.shape
        Ho, Wo = (H + 3) // 4, (W + 3) // 4
        M = N * Ho * Wo
        x = gemm(_a(_lib.SWIN_A_PATCH, img, n=N, c=C, h=H, w=W), M, p["k"], p["w"], shift=p["b"])
        if self.norm is not None:
            x = layernorm(x, self.norm)
        return x, (Ho, Wo)


class PatchMerging(nn.Module):
    """utils/transformer.py:260-400: Unfold(2, stride 2, corner padding) -> LayerNorm(4C) -> Linear(4C, 2C, no bias)"""

    def __init__(self, in_channels, out_channels, stride=2, norm_cfg=dict(type="LN")):
        super().__init__()
        if stride != 2:
            raise NotImplementedError(f"PatchMerging: stride {stride} (only 2 is built)")
        self.in_channels = in_channels
        self.out_channels = out_channels
        if norm_cfg is not None:
            _ln_only(norm_cfg)
            self.norm = nn.LayerNorm(4 * in_channels)
        else:
            self.norm = None
        self.reduction = nn.Linear(4 * in_channels, out_channels, bias=False)

    def pack(self, linear=PackedLinear):
        """linear: PackedLinear (default mode) or PackedLinearF16 (f16 inference mode)"""
        # nn.Unfold orders the merged vector c*4 + q (q = kh*2 + kw); the loader reads q*C + c (contiguous channels)
        C = self.in_channels
        w = self.reduction.weight.detach().float()
        wl = w.view(-1, C, 4).permute(0, 2, 1).reshape(w.shape[0], 4 * C)
        p = dict(w=linear(wl))
        if self.norm is not None:
            p["g"] = self.norm.weight.detach().float().view(C, 4).t().contiguous().view(-1)
            p["b"] = self.norm.bias.detach().float().view(C, 4).t().contiguous().view(-1)
        return p

    def run(self, p, x, B, H, W):
        C = self.in_channels
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
        M = B * Ho * Wo
        geo = dict(n=B, c=C, h=H, w=W)
        if self.norm is not None:
            st = row_stats(_a(_lib.SWIN_A_MERGE, x, **geo), M, 4 * C, self.norm.eps)
            a = _a(_lib.SWIN_A_MERGE, x, stats=st, ln=(p["g"], p["b"]), **geo)
        else:
            a = _a(_lib.SWIN_A_MERGE, x, **geo)
        return gemm(a,M, 4 * C, p["w"]), (Ho, Wo)


class SwinBlockSequence(nn.Module):
    """swin.py:371-455"""

    def __init__(self, embed_dims, num_heads, feedforward_channels, depth, window_size=7, qkv_bias=True,
                 qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0., downsample=None,
                 act_cfg=dict(type="GELU"), norm_cfg=dict(type="LN")):
        super().__init__()
        rates = drop_path_rate if isinstance(drop_path_rate, list) else [drop_path_rate] * depth
        assert len(rates) == depth
        self.blocks = nn.ModuleList([
            SwinBlock(embed_dims, num_heads, feedforward_channels, window_size, i % 2 == 1, qkv_bias, qk_scale,
                      drop_rate, attn_drop_rate, rates[i], act_cfg, norm_cfg) for i in range(depth)])
        self.downsample = downsample


class SwinTransformer(nn.Module):
    """swin.py:458-763 (BACKBONES 'SwinTransformer').  forward(x [N, 3, H, W]) -> [N, C_i, H_i, W_i] per out_index."""

    def __init__(self, pretrain_img_size=224, in_channels=3, embed_dims=96, patch_size=4, window_size=7, mlp_ratio=4,
                 depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), strides=(4, 2, 2, 2), out_indices=(0, 1, 2, 3),
                 qkv_bias=True, qk_scale=None, patch_norm=True, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1,
                 use_abs_pos_embed=False, act_cfg=dict(type="GELU"), norm_cfg=dict(type="LN"), with_cp=False,
                 pretrained=None, convert_weights=False, frozen_stages=-1, init_cfg=None):
        super().__init__()
        for flag, what in ((use_abs_pos_embed, "use_abs_pos_embed"), (with_cp, "with_cp"),
                           (convert_weights, "convert_weights"), (frozen_stages >= 0, "frozen_stages >= 0"),
                           (pretrained is not None, "pretrained"), (init_cfg is not None, "init_cfg")):
            if flag:
                raise NotImplementedError(f"SwinTransformer: {what} is not supported (load weights with "
                                          "load_state_dict instead)")
        _ln_only(norm_cfg)
        if window_size != 7:
            raise NotImplementedError(f"SwinTransformer: window_size {window_size} (only 7 is built)")
        for C, h in zip([embed_dims * 2 ** i for i in range(len(depths))], num_heads):
            if C != 32 * h:
                raise NotImplementedError(f"SwinTransformer: head dim {C / h} (only 32 is built)")
        assert strides[0] == patch_size, "Use non-overlapping patch embed."
        self.out_indices = out_indices
        self.use_abs_pos_embed = use_abs_pos_embed
        self.drop_rate, self.attn_drop_rate = drop_rate, attn_drop_rate
        self.patch_embed = PatchEmbed(in_channels, embed_dims, patch_size, strides[0],
                                      norm_cfg if patch_norm else None)
        self.drop_after_pos = nn.Dropout(p=drop_rate)
        total = sum(depths)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, total)]
        self.drop_path_rates = dpr          # per block, in block order
        self.stages = nn.ModuleList()
        c = embed_dims
        for i in range(len(depths)):
            down = (PatchMerging(c, 2 * c, strides[i + 1], norm_cfg if patch_norm else None)
                    if i < len(depths) - 1 else None)
            self.stages.append(SwinBlockSequence(c, num_heads[i], mlp_ratio * c, depths[i], window_size, qkv_bias,
                                                 qk_scale, drop_rate, attn_drop_rate,
                                                 dpr[sum(depths[:i]):sum(depths[:i + 1])], down, act_cfg, norm_cfg))
            if down is not None:
                c = down.out_channels
        self.num_features = [int(embed_dims * 2 ** i) for i in range(len(depths))]
        for i in out_indices:
            self.add_module(f"norm{i}", nn.LayerNorm(self.num_features[i]))

    PRECISIONS = ("f32", "f16")
    precision = "f32"       # a plain attribute (set_precision): not a parameter, buffer or constructor argument

    def set_precision(self, mode):
        """"f32": the default f16x3 kernels (fp32-class accuracy).  "f16": the f16 inference mode -- single-pass
        products, f16 branch intermediates, fp32 residual stream; eval-mode forward only."""
        if mode not in self.PRECISIONS:
            raise ValueError(f"SwinTransformer.set_precision: {mode!r} (one of {self.PRECISIONS})")
        self.precision = mode
        return self

    def _packed(self, dev):
        """the packed weights of the current mode; both modes' copies share the module's one derived-weight store, so a
        parameter change drops both and each is derived again on its next use"""
        c = _cache(self, dev)
        if self.precision not in c:
            linear = {"f32": PackedLinear, "f16": PackedLinearF16}[self.precision]
            with torch.no_grad():
                c[self.precision] = dict(
                    patch=self.patch_embed.pack(linear),
                    blocks=[[blk.pack(linear) for blk in st.blocks] for st in self.stages],
                    merge=[st.downsample.pack(linear) if st.downsample is not None else None for st in self.stages])
        return c[self.precision]

    @torch.no_grad()
    def forward(self, x):
        if self.training:
            raise _training_error("SwinTransformer")
        return self._run(x, None)

    def drop_layers(self):
        """DropPath rates of the layers that draw a mask, in mask-row order: by block, the attention branch before the
        FFN; a block whose rate is 0 draws nothing (mmcv DropPath returns its input)"""
        return [r for r in self.drop_path_rates if r > 0.0 for _ in range(2)]

    @torch.no_grad()
    def forward_train(self, x, drop_keep=None):
        """Training-mode forward: forward()'s kernels with stochastic depth (mmcv DropPath: per image keep =
        floor(keep_prob + U[0, 1)), branch output * keep / keep_prob).  No backward: the maps come back without a
        gradient (the shipped config detaches them).  drop_keep: [len(drop_layers()), N] of 0 / 1, one row per drawing
        layer in drop_layers() order; None draws every mask with ONE torch.rand call on the device (mmcv's random
        stream is not reproduced draw for draw)."""
        assert self.training, "call .train() first (forward() is the eval-mode forward)"
        if self.precision != "f32":
            raise NotImplementedError(f"SwinTransformer.forward_train: precision {self.precision!r} is an inference "
                                      'mode (train with set_precision("f32"))')
        if self.drop_rate != 0.0 or self.attn_drop_rate != 0.0:
            raise NotImplementedError(f"SwinTransformer.forward_train: drop_rate {self.drop_rate} / attn_drop_rate "
                                      f"{self.attn_drop_rate} (only DropPath is built)")
        _lib.require_cuda(x)
        rates = self.drop_layers()
        if not rates:
            return self._run(x, None)
        N = x.shape[0]
        keep_prob = 1.0 - torch.tensor(rates, dtype=torch.float32, device=x.device)[:, None]
        if drop_keep is None:
            drop_keep = torch.floor(keep_prob + torch.rand(len(rates), N, device=x.device))
        else:
            _lib.require_cuda(drop_keep)
            if tuple(drop_keep.shape) != (len(rates), N):
                raise ValueError(f"drop_keep {tuple(drop_keep.shape)}: need {(len(rates), N)}")
        return self._run(x, (drop_keep.to(torch.float32) / keep_prob).contiguous())

    def _run(self, x, scales):
        """scales: [len(drop_layers()), N] DropPath factors (keep / keep_prob) or None"""
        _lib.require_cuda(x)
        assert x.dim() == 4, x.shape
        x = x.float().contiguous()
        N = x.shape[0]
        assert scales is None or self.precision == "f32"      # DropPath is not built for the f16 inference mode
        p = self._packed(x.device)
        t, (H, W) = self.patch_embed.run(p["patch"], x)
        outs = []
        row = 0
        for i, stage in enumerate(self.stages):
            for blk, bp in zip(stage.blocks, p["blocks"][i]):
                keep = (None, None)
                if scales is not None and blk.attn.drop_path_rate > 0.0:
                    keep = (scales[row], scales[row + 1])
                    row += 2
                t = blk.run(bp, t, N, H, W, keep)
            if i in self.out_indices:
                outs.append(layernorm(t, getattr(self, f"norm{i}"), out_nchw=(N, H, W)))
            if stage.downsample is not None:
                t, (H, W) = stage.downsample.run(p["merge"][i], t, N, H, W)
        return outs
