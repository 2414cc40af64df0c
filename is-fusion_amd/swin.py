"""Camera backbone: the reference's SwinTransformer (mmdet3d/models/backbones/swin.py, with PatchEmbed / PatchMerging of
models/utils/transformer.py) on the HIP kernels of isf_swin.hip.  ``forward`` is the eval-mode forward;
``forward_train`` is the training-mode forward (stochastic depth).  By default it has no backward: the shipped config
detaches the backbone's outputs (``detach=True``, isfusion.py:76-77), so training needs no gradient through it.
``forward_train(..., backward=True)`` runs the same launches and hangs ONE autograd node on the maps whose backward is
built from the kernels of isf_swin_train.hip (window-attention, LayerNorm and GELU backward, fixed-order column sums) and
from the forward's own GEMM on transposed packed weights (dX) and isf_rows_weight_grad (dW); DESIGN.md section 4.0c.

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

``set_precision("mixed")`` is mixed-precision training: in eval() it is the f16 mode bit for bit (the same packed
weights), in train() ``forward_train`` runs the f16 block with the DropPath factor in the proj / fc2 epilogue
(isf_swin_gemm_f16_rowscale) and keeps, per block, the fp32 rows x and y, both LayerNorms' statistics and the f16 qkv
rows and attention output.  The backward is the f32 mode's schedule with single-pass products: dX on the f16 pack of the
transposed weight, dW by isf_rows_weight_grad_f16, the window attention by isf_swin_window_attention_backward_f16
(isf_swin_train_f16.hip); gradient rows, LayerNorm / GELU backward, column sums and every parameter gradient stay fp32.
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


def gemm_f16_rowscale(a, rows, k, pl, row_scale, *, shift=None, residual=None):
    """isf_swin_gemm_f16_rowscale: (A W^T + shift) * row_scale[sample of the row] + residual -> fp32 rows [rows, N], for
    f16 A rows and a PackedLinearF16 (the proj / fc2 epilogue of mixed-precision training, DropPath)"""
    s, keep = a
    x, N = keep[0], pl.out_features
    assert isinstance(pl, PackedLinearF16) and x.dtype == torch.float16
    assert row_scale.dtype == torch.float32 and row_scale.is_contiguous() and rows % row_scale.numel() == 0
    assert residual is None or (residual.dtype == torch.float32 and residual.is_contiguous()
                                and tuple(residual.shape) == (rows, N))
    y = torch.empty((rows, N), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().isf_swin_gemm_f16_rowscale(
        ctypes.byref(s), 1, rows, k, _lib.ptr(pl.packed), N, None, _lib.ptr(shift), ACT_NONE, _lib.ptr(residual),
        _lib.ptr(row_scale), rows // row_scale.numel(), _lib.ptr(y), 0, N, 0, _lib.stream()), "isf_swin_gemm_f16_rowscale")
    return y


def _branch_out(a, rows, k, pl, shift, residual, row_scale):
    """the Linear that closes a block's branch: + bias, DropPath factor (or None), + identity"""
    if row_scale is not None and isinstance(pl, PackedLinearF16):
        return gemm_f16_rowscale(a, rows, k, pl, row_scale, shift=shift, residual=residual)
    return gemm(a, rows, k, pl, shift=shift, residual=residual, row_scale=row_scale)


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


# ------------------------------------------------------------------------------------------- backward (isf_swin_train.hip)
def operand_rows(a, rows, k):
    """isf_swin_operand_rows: the loader's operand rows written out, [rows, k] (after its LayerNorm prologue, if any)"""
    s, keep = a
    out = torch.empty((rows, k), dtype=torch.float32, device=keep[0].device)
    _lib.check(_lib.load().isf_swin_operand_rows(ctypes.byref(s), rows, k, _lib.ptr(out), _lib.stream()),
               "isf_swin_operand_rows")
    return out


def layernorm_backward(a, rows, k, dy, *, dy_hw=0, dy_scale=None, residual=None, dx_shape=None, inv_scale=None):
    """isf_swin_layernorm_backward over the loader's rows (ROWS or MERGE with stats and gamma) -> (dx, dgamma, dbeta).
    dy: rows [rows, k], or an NCHW map [B, k, H, W] with dy_hw = H * W; dy_scale / inv_scale: device scalars (factor on
    dy / on dgamma and dbeta) or None; residual: rows added to dx (ROWS); dx_shape: the token rows a MERGE loader
    gathers from (default [rows, k])."""
    s, keep = a
    _lib.require_cuda(dy)
    assert dy.dtype == torch.float32 and dy.is_contiguous() and dy.numel() == rows * k
    assert residual is None or (residual.dtype == torch.float32 and residual.is_contiguous()
                                and tuple(residual.shape) == (rows, k))
    dev = dy.device
    dx = torch.empty(dx_shape or (rows, k), dtype=torch.float32, device=dev)
    lib = _lib.load()
    parts = lib.isf_swin_layernorm_backward_parts(rows)
    ws = torch.empty((parts, 2, k), dtype=torch.float32, device=dev)
    dg, db = torch.empty(k, dtype=torch.float32, device=dev), torch.empty(k, dtype=torch.float32, device=dev)
    _lib.check(lib.isf_swin_layernorm_backward(ctypes.byref(s), rows, k, _lib.ptr(dy), dy_hw, _lib.ptr(dy_scale),
                                               _lib.ptr(residual), _lib.ptr(dx), _lib.ptr(inv_scale), _lib.ptr(ws), parts,
                                               _lib.ptr(dg), _lib.ptr(db), _lib.stream()), "isf_swin_layernorm_backward")
    return dx, dg, db


def column_sums(g, extra=None, inv_scale=None):
    """isf_swin_column_sums: inv_scale * (g.sum(0) + extra) in a fixed order"""
    _lib.require_cuda(g)
    assert g.dtype == torch.float32 and g.is_contiguous() and g.dim() == 2
    M, N = g.shape
    lib = _lib.load()
    parts = lib.isf_swin_column_sums_parts(M)
    ws = torch.empty((parts, N), dtype=torch.float32, device=g.device)
    out = torch.empty(N, dtype=torch.float32, device=g.device)
    _lib.check(lib.isf_swin_column_sums(_lib.ptr(g), M, N, _lib.ptr(extra), _lib.ptr(inv_scale), _lib.ptr(ws), parts,
                                        _lib.ptr(out), _lib.stream()), "isf_swin_column_sums")
    return out


def gelu_backward(hidden, grad):
    """isf_swin_gelu_backward, in place: hidden (pre-activation) -> gelu(hidden), grad -> grad * gelu'(hidden)"""
    assert hidden.dtype == grad.dtype == torch.float32 and hidden.is_contiguous() and grad.is_contiguous()
    assert hidden.shape == grad.shape
    _lib.check(_lib.load().isf_swin_gelu_backward(_lib.ptr(hidden), _lib.ptr(grad), hidden.numel(), _lib.stream()),
               "isf_swin_gelu_backward")


def scale_rows(g, row_scale):
    """isf_swin_scale_rows: g [M, N] * row_scale[sample of the row] (DropPath on a gradient); None passes g through"""
    if row_scale is None:
        return g
    M, N = g.shape
    assert g.dtype == torch.float32 and g.is_contiguous() and M % row_scale.numel() == 0
    out = torch.empty_like(g)
    _lib.check(_lib.load().isf_swin_scale_rows(_lib.ptr(g), M, N, _lib.ptr(row_scale), M // row_scale.numel(),
                                               _lib.ptr(out), _lib.stream()), "isf_swin_scale_rows")
    return out


def window_attention_backward(qkv, qkv_bias, rel_bias, dout, B, H, W, C, heads, window, shift, scale, rel_index=None,
                              table_rows=0, inv_scale=None):
    """isf_swin_window_attention_backward: gradient rows dout [B*H*W, C] of window_attention's output ->
    (dqkv [B*H*W, 3C], drel_bias [heads, 49, 49], dtable [table_rows, heads] * inv_scale or None (without rel_index),
    the padded cells' share of the qkv-bias gradient [3C]), all fp32.  f16 qkv rows (the f16 forward's) go to
    isf_swin_window_attention_backward_f16."""
    _lib.require_cuda(qkv, dout)
    M = B * H * W
    entry = {torch.float32: "isf_swin_window_attention_backward",
             torch.float16: "isf_swin_window_attention_backward_f16"}[qkv.dtype]
    assert qkv.is_contiguous() and tuple(qkv.shape) == (M, 3 * C)
    assert dout.dtype == torch.float32 and dout.is_contiguous() and tuple(dout.shape) == (M, C)
    dev = qkv.device
    lib = _lib.load()
    groups = lib.isf_swin_window_attention_backward_groups(B, H, W, heads)
    n = window * window
    ws = torch.empty(groups * heads * (n * n + 64), dtype=torch.float32, device=dev)
    dqkv = torch.empty((M, 3 * C), dtype=torch.float32, device=dev)
    drel = torch.empty((heads, n, n), dtype=torch.float32, device=dev)
    dtable = torch.empty((table_rows, heads), dtype=torch.float32, device=dev) if rel_index is not None else None
    pad = torch.empty(3 * C, dtype=torch.float32, device=dev)
    if rel_index is not None:
        assert rel_index.dtype == torch.int64 and rel_index.is_contiguous() and rel_index.numel() == n * n
    _lib.check(getattr(lib, entry)(
        _lib.ptr(qkv), _lib.ptr(qkv_bias), _lib.ptr(rel_bias), _lib.ptr(rel_index), _lib.ptr(dout), B, H, W, C, heads,
        window, shift, float(scale), _lib.ptr(inv_scale), _lib.ptr(ws), groups, _lib.ptr(dqkv), _lib.ptr(drel),
        _lib.ptr(dtable), table_rows, _lib.ptr(pad), _lib.stream()), entry)
    return dqkv, drel, dtable, pad


def _rows_weight_grad(g, x, inv_scale, f16=False):
    if f16:
        return rows_weight_grad_f16(g, x, inv_scale)
    from .generalized_lss import rows_weight_grad       # (generalized_lss imports this module)
    return rows_weight_grad(g, x, inv_scale)


def rows_weight_grad_f16(g, x, inv_scale=None):
    """isf_rows_weight_grad_f16: dW [N, K] = inv_scale * g^T x with single-pass products, for fp32 gradient rows g [R, N]
    and token rows x [R, K], fp32 or f16 (both rounded to f16 in the kernel; fp32 accumulation)"""
    _lib.require_cuda(g, x)
    assert g.dtype == torch.float32 and x.dtype in (torch.float32, torch.float16) and g.is_contiguous()
    assert x.is_contiguous() and x.dim() == 2 and x.shape[0] == g.shape[0]
    (R, N), K = g.shape, x.shape[1]
    lib = _lib.load()
    chunks = lib.isf_rows_weight_grad_chunks(R, N, K)
    ws = torch.empty((chunks, N, K), dtype=torch.float32, device=g.device)
    out = torch.empty((N, K), dtype=torch.float32, device=g.device)
    _lib.check(lib.isf_rows_weight_grad_f16(_lib.ptr(g), _lib.ptr(x), int(x.dtype == torch.float16), K, R, N, K,
                                            _lib.ptr(inv_scale), _lib.ptr(ws), chunks, _lib.ptr(out), K, _lib.stream()),
               "isf_rows_weight_grad_f16")
    return out


def _pack_transposed(weight, linear):
    """W [out, in] packed for dX = dY . W: PackedLinear packs the transpose itself, PackedLinearF16 takes W^T"""
    if linear is PackedLinearF16:
        return PackedLinearF16(weight.detach().float().t().contiguous())
    return linear(weight, transposed=True)


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

    def pack_backward(self, linear=PackedLinear):
        """the transposed packed weights of dX = dY . W, one per Linear; linear as in pack()"""
        m = self.attn.w_msa
        l1, l2 = self.ffn.layers[0][0], self.ffn.layers[1]
        return {name: _pack_transposed(w, linear)
                for name, w in (("qkv", m.qkv.weight), ("proj", m.proj.weight), ("fc1", l1.weight), ("fc2", l2.weight))}

    def run(self, p, x, B, H, W, keep=(None, None), tape=None):
        """x: token rows [B*H*W, C] -> the block's output rows; x and the result are the fp32 residual rows.  With the
        f16 pack (pack(PackedLinearF16)) qkv, the attention output and the FFN hidden are f16 rows.  keep: per-image
        DropPath factors [B] (keep / keep_prob) of the attention and the FFN branch, or None: the branch output is
        multiplied by them after window reverse / un-shift and before the identity is added (swin.py:251, mmcv FFN);
        with the f16 pack they go through gemm_f16_rowscale (mixed-precision training).  tape: a list that receives what
        run_backward needs (the same launches either way)."""
        M, C = x.shape
        m = self.attn.w_msa
        h16 = isinstance(p["qkv"], PackedLinearF16)
        ln1 = (self.norm1.weight.detach(), self.norm1.bias.detach())
        st = row_stats(_a(_lib.SWIN_A_ROWS, x, ldx=C), M, C, self.norm1.eps)
        qkv = gemm(_a(_lib.SWIN_A_ROWS, x, ldx=C, stats=st, ln=ln1), M, C, p["qkv"], shift=p["qkv_b"], out_f16=h16)
        att = window_attention(qkv, p["qkv_b"], p["rel"], B, H, W, C, m.num_heads, self.attn.window_size,
                               self.attn.shift_size, m.scale)
        rec = None if tape is None else dict(x=x, st1=st, qkv=qkv, att=att, keep=keep)
        x = _branch_out(_a(_lib.SWIN_A_ROWS, att, ldx=C), M, C, p["proj"], p["proj_b"], x, keep[0])
        ln2 = (self.norm2.weight.detach(), self.norm2.bias.detach())
        st = row_stats(_a(_lib.SWIN_A_ROWS, x, ldx=C), M, C, self.norm2.eps)
        F = self.ffn.feedforward_channels
        h = gemm(_a(_lib.SWIN_A_ROWS, x, ldx=C, stats=st, ln=ln2), M, C, p["fc1"], shift=p["fc1_b"], act=ACT_GELU,
                 out_f16=h16)
        if tape is not None:
            rec.update(y=x, st2=st)
            tape.append(rec)
        return _branch_out(_a(_lib.SWIN_A_ROWS, h, ldx=F), M, F, p["fc2"], p["fc2_b"], x, keep[1])

    def run_backward(self, p, pb, rec, g, B, H, W, inv, grads):
        """g: gradient rows [B*H*W, C] of the block's output, pre-scaled (1 / inv[0] is the scale) -> the gradient rows
        of its input in the same scale; the twelve parameter gradients (times inv) go into grads[parameter].
        rec: what run() left on the tape -- the block's input x, the rows y between its branches, both LayerNorms'
        (mean, rstd) rows, the qkv rows and the attention output.  The FFN's hidden rows are not kept: the first Linear
        runs again (without GELU) and isf_swin_gelu_backward turns them into gelu(.) and the gradient into dL/dz.
        With the f16 packs (mixed precision) every product is single-pass and rec's qkv / attention rows are f16; the
        gradient rows, the recomputed hidden and everything that is not a product stay fp32."""
        M, C = g.shape
        h16 = isinstance(p["qkv"], PackedLinearF16)
        m = self.attn.w_msa
        l1, l2 = self.ffn.layers[0][0], self.ffn.layers[1]
        F = self.ffn.feedforward_channels
        rows = lambda t: _a(_lib.SWIN_A_ROWS, t, ldx=t.shape[1])
        # FFN branch: out = y + keep1 * (gelu(LN2(y) W1^T + b1) W2^T + b2)
        y, x = rec["y"], rec["x"]
        ln2 = (self.norm2.weight.detach(), self.norm2.bias.detach())
        a2 = _a(_lib.SWIN_A_ROWS, y, ldx=C, stats=rec["st2"], ln=ln2)
        df = scale_rows(g, rec["keep"][1])
        h = gemm(a2, M, C, p["fc1"], shift=p["fc1_b"])
        dh = gemm(rows(df), M, C, pb["fc2"])
        gelu_backward(h, dh)
        grads[l2.weight] = _rows_weight_grad(df, h, inv, h16)
        grads[l2.bias] = column_sums(df, inv_scale=inv)
        del h
        grads[l1.weight] = _rows_weight_grad(dh, operand_rows(a2, M, C), inv, h16)
        grads[l1.bias] = column_sums(dh, inv_scale=inv)
        dn = gemm(rows(dh), M, F, pb["fc1"])
        del dh
        dy, grads[self.norm2.weight], grads[self.norm2.bias] = layernorm_backward(a2, M, C, dn, residual=g,
                                                                                  inv_scale=inv)
        # attention branch: y = x + keep0 * (attention(LN1(x) Wqkv^T + bqkv) Wp^T + bp)
        dp = scale_rows(dy, rec["keep"][0])
        grads[m.proj.weight] = _rows_weight_grad(dp, rec["att"], inv, h16)
        grads[m.proj.bias] = column_sums(dp, inv_scale=inv)
        datt = gemm(rows(dp), M, C, pb["proj"])
        table = m.relative_position_bias_table
        dqkv, _, grads[table], pad = window_attention_backward(
            rec["qkv"], p["qkv_b"], p["rel"], datt, B, H, W, C, m.num_heads, self.attn.window_size, self.attn.shift_size,
            m.scale, rel_index=m.relative_position_index, table_rows=table.shape[0], inv_scale=inv)
        ln1 = (self.norm1.weight.detach(), self.norm1.bias.detach())
        a1 = _a(_lib.SWIN_A_ROWS, x, ldx=C, stats=rec["st1"], ln=ln1)
        grads[m.qkv.weight] = _rows_weight_grad(dqkv, operand_rows(a1, M, C), inv, h16)
        if m.qkv.bias is not None:
            grads[m.qkv.bias] = column_sums(dqkv, extra=pad, inv_scale=inv)
        dn = gemm(rows(dqkv), M, 3 * C, pb["qkv"])
        dx, grads[self.norm1.weight], grads[self.norm1.bias] = layernorm_backward(a1, M, C, dn, residual=dy,
                                                                                  inv_scale=inv)
        return dx


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

    def run(self, p, img, tape=None):
        N, C, H, W = img.shape
        Ho, Wo = (H + 3) // 4, (W + 3) // 4
        M = N * Ho * Wo
        x = gemm(_a(_lib.SWIN_A_PATCH, img, n=N, c=C, h=H, w=W), M, p["k"], p["w"], shift=p["b"])
        if tape is not None:
            tape.append(dict(img=img, raw=x))
        if self.norm is not None:
            x = layernorm(x, self.norm)
        return x, (Ho, Wo)

    def run_backward(self, rec, g, cum, grads, f16=False):
        """g: gradient rows of run()'s output times cum[0] -> the projection's (and the norm's) gradients; the image
        gets none.  dW = dY^T . patches on the im2col rows (isf_swin_operand_rows, PATCH); f16: single-pass products."""
        img, raw = rec["img"], rec["raw"]
        N, C, H, W = img.shape
        M, E = raw.shape
        inv = cum[1:]
        if self.norm is not None:
            st = row_stats(_a(_lib.SWIN_A_ROWS, raw, ldx=E), M, E, self.norm.eps)
            a = _a(_lib.SWIN_A_ROWS, raw, ldx=E, stats=st, ln=(self.norm.weight.detach(), self.norm.bias.detach()))
            g, grads[self.norm.weight], grads[self.norm.bias] = layernorm_backward(a, M, E, g, inv_scale=inv)
        patches = operand_rows(_a(_lib.SWIN_A_PATCH, img, n=N, c=C, h=H, w=W), M, 16 * C)
        grads[self.projection.weight] = _rows_weight_grad(g, patches, inv, f16).view(self.projection.weight.shape)
        grads[self.projection.bias] = column_sums(g, inv_scale=inv)


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

    def run(self, p, x, B, H, W, tape=None):
        C = self.in_channels
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
        M = B * Ho * Wo
        geo = dict(n=B, c=C, h=H, w=W)
        if self.norm is not None:
            st = row_stats(_a(_lib.SWIN_A_MERGE, x, **geo), M, 4 * C, self.norm.eps)
            a = _a(_lib.SWIN_A_MERGE, x, stats=st, ln=(p["g"], p["b"]), **geo)
        else:
            st = None
            a = _a(_lib.SWIN_A_MERGE, x, **geo)
        if tape is not None:
            tape.append(dict(x=x, st=st))
        return gemm(a,M, 4 * C, p["w"]), (Ho, Wo)

    def pack_backward(self, p, linear=PackedLinear):
        """the transposed packed reduction weight, in the loader's column order; linear as in pack()"""
        C = self.in_channels
        w = self.reduction.weight.detach().float()
        return _pack_transposed(w.view(-1, C, 4).permute(0, 2, 1).reshape(w.shape[0], 4 * C).contiguous(), linear)

    def run_backward(self, p, pb, rec, g, B, H, W, inv, grads):
        """g: gradient rows [B*Ho*Wo, 2C] of run()'s output (pre-scaled; inv as in SwinBlock.run_backward) -> the
        gradient of the token rows [B*H*W, C].  The LayerNorm backward writes dx on the token rows: that is the adjoint
        of the 2 x 2 gather, and the gradient of corner padding is dropped.  Gradients are computed in the loader's
        q*C + c column order and handed out in nn.Unfold's c*4 + q."""
        if self.norm is None:
            raise NotImplementedError("PatchMerging: backward without the LayerNorm (norm_cfg=None) is not built")
        x = rec["x"]
        C = self.in_channels
        M, N = g.shape
        a = _a(_lib.SWIN_A_MERGE, x, stats=rec["st"], ln=(p["g"], p["b"]), n=B, c=C, h=H, w=W)
        dw = _rows_weight_grad(g, operand_rows(a, M, 4 * C), inv, isinstance(pb, PackedLinearF16))
        grads[self.reduction.weight] = dw.view(N, 4, C).permute(0, 2, 1).reshape(N, 4 * C)
        dn = gemm(_a(_lib.SWIN_A_ROWS, g, ldx=N), M, N, pb)
        dx, dg, db = layernorm_backward(a, M, 4 * C, dn, dx_shape=tuple(x.shape), inv_scale=inv)
        grads[self.norm.weight] = dg.view(4, C).t().reshape(-1)
        grads[self.norm.bias] = db.view(4, C).t().reshape(-1)
        return dx


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

    PRECISIONS = ("f32", "f16", "mixed")
    precision = "f32"       # a plain attribute (set_precision): not a parameter, buffer or constructor argument

    def set_precision(self, mode):
        """"f32": the default f16x3 kernels (fp32-class accuracy).  "f16": the f16 inference mode -- single-pass
        products, f16 branch intermediates, fp32 residual stream; eval-mode forward only.  "mixed": mixed-precision
        training -- the f16 mode's forward in eval(), and in train() forward_train with f16 products, f16 saved qkv /
        attention rows, fp32 residual stream, statistics, softmax and parameter gradients."""
        if mode not in self.PRECISIONS:
            raise ValueError(f"SwinTransformer.set_precision: {mode!r} (one of {self.PRECISIONS})")
        self.precision = mode
        return self

    def _packed(self, dev):
        """the packed weights of the current mode; both modes' copies share the module's one derived-weight store, so a
        parameter change drops both and each is derived again on its next use"""
        c = _cache(self, dev)
        key = self._PACKS[self.precision]      # "mixed" runs on the f16 mode's packed weights
        if key not in c:
            linear = {"f32": PackedLinear, "f16": PackedLinearF16}[key]
            with torch.no_grad():
                c[key] = dict(
                    patch=self.patch_embed.pack(linear),
                    blocks=[[blk.pack(linear) for blk in st.blocks] for st in self.stages],
                    merge=[st.downsample.pack(linear) if st.downsample is not None else None for st in self.stages])
        return c[key]

    _PACKS = {"f32": "f32", "f16": "f16", "mixed": "f16"}

    @torch.no_grad()
    def forward(self, x):
        if self.training:
            raise _training_error("SwinTransformer")
        return self._run(x, None)

    def drop_layers(self):
        """DropPath rates of the layers that draw a mask, in mask-row order: by block, the attention branch before the
        FFN; a block whose rate is 0 draws nothing (mmcv DropPath returns its input)"""
        return [r for r in self.drop_path_rates if r > 0.0 for _ in range(2)]

    def forward_train(self, x, drop_keep=None, backward=False):
        """Training-mode forward: forward()'s kernels with stochastic depth (mmcv DropPath: per image keep =
        floor(keep_prob + U[0, 1)), branch output * keep / keep_prob).  backward=False: no backward, the maps come back
        without a gradient (the shipped config detaches them).  backward=True: the same launches, and the maps carry ONE
        autograd node (_SwinBackward) whose backward runs the kernels of isf_swin_train.hip and hands fp32 gradients to
        the backbone's parameters; the image gets none.  drop_keep: [len(drop_layers()), N] of 0 / 1, one row per
        drawing layer in drop_layers() order; None draws every mask with ONE torch.rand call on the device (mmcv's
        random stream is not reproduced draw for draw)."""
        with torch.no_grad():
            x, scales = self._train_inputs(x, drop_keep)
            if not backward:
                return self._run(x, scales)
        params = [q for q in self.parameters() if q.requires_grad]
        return list(_SwinBackward.apply(self, x.detach(), scales, *params))

    def _train_inputs(self, x, drop_keep):
        """forward_train's checks -> (x, the DropPath factors [len(drop_layers()), N] or None)"""
        assert self.training, "call .train() first (forward() is the eval-mode forward)"
        if self.precision == "f16":
            raise NotImplementedError(f"SwinTransformer.forward_train: precision {self.precision!r} is an inference "
                                      'mode (train with set_precision("f32") or set_precision("mixed"))')
        if self.drop_rate != 0.0 or self.attn_drop_rate != 0.0:
            raise NotImplementedError(f"SwinTransformer.forward_train: drop_rate {self.drop_rate} / attn_drop_rate "
                                      f"{self.attn_drop_rate} (only DropPath is built)")
        _lib.require_cuda(x)
        rates = self.drop_layers()
        if not rates:
            return x, None
        N = x.shape[0]
        keep_prob = 1.0 - torch.tensor(rates, dtype=torch.float32, device=x.device)[:, None]
        if drop_keep is None:
            drop_keep = torch.floor(keep_prob + torch.rand(len(rates), N, device=x.device))
        else:
            _lib.require_cuda(drop_keep)
            if tuple(drop_keep.shape) != (len(rates), N):
                raise ValueError(f"drop_keep {tuple(drop_keep.shape)}: need {(len(rates), N)}")
        return x, (drop_keep.to(torch.float32) / keep_prob).contiguous()

    def _run(self, x, scales, tape=None):
        """scales: [len(drop_layers()), N] DropPath factors (keep / keep_prob) or None.  tape: a dict that receives what
        _run_backward needs (the launches are the same with and without it)."""
        _lib.require_cuda(x)
        assert x.dim() == 4, x.shape
        x = x.float().contiguous()
        N = x.shape[0]
        assert scales is None or self.precision in ("f32", "mixed")      # the f16 mode is inference only
        p = self._packed(x.device)
        if tape is not None:
            tape.update(n=N, patch=[], stages=[], precision=self.precision)
        t, (H, W) = self.patch_embed.run(p["patch"], x, None if tape is None else tape["patch"])
        outs = []
        row = 0
        for i, stage in enumerate(self.stages):
            blocks, merge = (None, None) if tape is None else ([], [])
            for blk, bp in zip(stage.blocks, p["blocks"][i]):
                keep = (None, None)
                if scales is not None and blk.attn.drop_path_rate > 0.0:
                    keep = (scales[row], scales[row + 1])
                    row += 2
                t = blk.run(bp, t, N, H, W, keep, blocks)
            if tape is not None:
                tape["stages"].append(dict(blocks=blocks, merge=merge, out=t, hw=(H, W)))
            if i in self.out_indices:
                outs.append(layernorm(t, getattr(self, f"norm{i}"), out_nchw=(N, H, W)))
            if stage.downsample is not None:
                t, (H, W) = stage.downsample.run(p["merge"][i], t, N, H, W, merge)
        return outs

    def _packed_backward(self, dev):
        """the transposed packed weights of the backward's dX = dY . W products, in the same derived-weight store as the
        forward's: a parameter update drops both"""
        c = _cache(self, dev)
        key = self._PACKS[self.precision] + "_backward"
        if key not in c:
            p = self._packed(dev)
            linear = PackedLinearF16 if key == "f16_backward" else PackedLinear
            with torch.no_grad():
                c[key] = dict(
                    blocks=[[blk.pack_backward(linear) for blk in st.blocks] for st in self.stages],
                    merge=[st.downsample.pack_backward(p["merge"][i], linear) if st.downsample is not None else None
                           for i, st in enumerate(self.stages)])
        return c[key]

    @torch.no_grad()
    def _run_backward(self, tape, gouts):
        """gouts: the gradient (or None) of each map _run returned, NCHW -> {parameter: fp32 gradient} for the
        parameters a gradient reaches.  The stream gradient g is carried pre-scaled by a power of two, renewed at every
        block's entry (_lib.grad_rescale: the f16 hi / lo products want operands near 2^10, gradients are 1e-5 and
        below); cum = [scale, 1 / scale] of g against the true gradient."""
        dev = tape["stages"][0]["out"].device
        if tape["precision"] != self.precision:
            raise RuntimeError(f"SwinTransformer: the forward ran in precision {tape['precision']!r}, the backward is "
                               f"asked for in {self.precision!r} (set_precision between forward_train and backward)")
        p, pb = self._packed(dev), self._packed_backward(dev)
        N = tape["n"]
        gmaps = dict(zip([i for i in range(len(self.stages)) if i in self.out_indices], gouts))
        grads = {}
        cum = torch.ones(2, dtype=torch.float32, device=dev)
        g = None
        for i in reversed(range(len(self.stages))):
            stage, rec = self.stages[i], tape["stages"][i]
            H, W = rec["hw"]
            t = rec["out"]
            M, C = t.shape
            if g is not None:          # from the stage above, through this stage's PatchMerging
                g = stage.downsample.run_backward(p["merge"][i], pb["merge"][i], rec["merge"][0], g, N, H, W, cum[1:], grads)
            go = gmaps.get(i)
            if go is not None:
                norm = getattr(self, f"norm{i}")
                _lib.require_cuda(go)
                st = row_stats(_a(_lib.SWIN_A_ROWS, t, ldx=C), M, C, norm.eps)
                a = _a(_lib.SWIN_A_ROWS, t, ldx=C, stats=st, ln=(norm.weight.detach(), norm.bias.detach()))
                g, grads[norm.weight], grads[norm.bias] = layernorm_backward(
                    a, M, C, go.float().contiguous(), dy_hw=H * W, dy_scale=cum[:1], residual=g, inv_scale=cum[1:])
            if g is None:
                continue
            for blk, bp, bpb, brec in reversed(list(zip(stage.blocks, p["blocks"][i], pb["blocks"][i], rec["blocks"]))):
                g, sc = _lib.grad_rescale(g)
                cum = cum * sc
                g = blk.run_backward(bp, bpb, brec, g, N, H, W, cum[1:], grads)
        if g is not None:
            self.patch_embed.run_backward(tape["patch"][0], g, cum, grads, f16=self.precision == "mixed")
        return grads


class _SwinBackward(torch.autograd.Function):
    """SwinTransformer._run with a backward: one node for the whole backbone (the training step is paced by the host).
    Inputs: the module, the image batch (no gradient), the DropPath factors, and the parameters (so that autograd routes
    their gradients); outputs: the out_indices maps."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, mod, x, scales, *params):
        tape = {}
        outs = mod._run(x, scales, tape)
        ctx.mod, ctx.tape, ctx.params = mod, tape, params
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gouts):
        grads = ctx.mod._run_backward(ctx.tape, gouts)
        ctx.tape = None
        return (None, None, None) + tuple(grads.get(q) for q in ctx.params)
