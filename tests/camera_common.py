"""Float64 torch restatement of the camera branch (SwinTransformer + GeneralizedLSSFPN of
configs/isfusion/isfusion_0075voxel.py) and the seeded weights the goldens and tests share.

The restatement is written from the modules' documented semantics with stock torch ops (conv2d, layer_norm, linear,
F.pad, torch.roll, nn.Unfold, F.interpolate); it runs in any dtype on any device.  tests/test_camera.py pins it to
tests/golden/camera_ref.npz (made by the reference's own modules), and the GPU tests use it as the full-size yardstick.
"""
import numpy as np
import torch
import torch.nn.functional as F

BACKBONE = dict(embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7, mlp_ratio=4,
                qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.2, patch_norm=True,
                out_indices=[1, 2, 3], with_cp=False, convert_weights=False)
NECK = dict(in_channels=[192, 384, 768], out_channels=256, start_level=0, num_outs=3)
GOLDEN_SIZES = ((2, 128, 352), (1, 90, 150))   # (images, H, W): even stage grids / odd grids (merge + patch padding)


def seeded_state_dict(shapes, seed):
    """{key: tensor} for an ordered {key: (shape, dtype)}: a numpy RandomState(seed) draws every floating entry in key
    order; integer buffers (relative_position_index, num_batches_tracked) are kept as given (value tensors).  Scales
    keep activations O(1) through 12 residual blocks: Linear / conv weights N(0, 1/fan_in), biases and LayerNorm shifts
    N(0, 0.1^2), LayerNorm / BN gains 1 + N(0, 0.1^2), relative position tables N(0, 0.5^2), BN running_var in
    [0.5, 1.5)."""
    rng = np.random.RandomState(seed)
    out = {}
    for k, v in shapes.items():
        if not torch.is_tensor(v) or v.dtype.is_floating_point is False:
            out[k] = v
            continue
        shape = tuple(v.shape)
        leaf = k.rsplit(".", 1)[-1]
        if leaf == "relative_position_bias_table":
            a = rng.normal(0.0, 0.5, shape)
        elif leaf == "running_var":
            a = rng.uniform(0.5, 1.5, shape)
        elif leaf == "running_mean" or leaf == "bias":
            a = rng.normal(0.0, 0.1, shape)
        elif leaf == "weight" and len(shape) == 1:
            a = 1.0 + rng.normal(0.0, 0.1, shape)
        else:
            fan_in = int(np.prod(shape[1:]))
            a = rng.normal(0.0, 1.0 / np.sqrt(fan_in), shape)
        out[k] = torch.from_numpy(a.astype(np.float32))
    return out


def seeded_module_state(module, seed):
    """seeded_state_dict over a module's own state_dict (keys, shapes, integer buffers)"""
    return seeded_state_dict(module.state_dict(), seed)


def images(seed, n, h, w):
    return torch.from_numpy(np.random.RandomState(seed).normal(0.0, 1.0, (n, 3, h, w)).astype(np.float32))


# ---------------------------------------------------------------------------------------------------- restatement
def _rel_bias(sd, p, heads, ws):
    n = ws * ws
    idx = sd[p + "relative_position_index"].view(-1).long()
    return sd[p + "relative_position_bias_table"][idx].view(n, n, heads).permute(2, 0, 1)


def _windows(x, ws):
    B, H, W, C = x.shape
    return x.view(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)


def _unwindows(w, B, H, W, ws):
    C = w.shape[-1]
    return w.view(B, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)


def shift_window_msa(sd, p, x, hw, heads, ws, shift):
    """ShiftWindowMSA on token rows x [B, L, C] (after norm1)"""
    B, L, C = x.shape
    H, W = hw
    x = x.view(B, H, W, C)
    pr, pb = (ws - W % ws) % ws, (ws - H % ws) % ws
    x = F.pad(x, (0, 0, 0, pr, 0, pb))
    Hp, Wp = x.shape[1], x.shape[2]
    mask = None
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
        lab = torch.zeros((1, Hp, Wp, 1), dtype=x.dtype, device=x.device)
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                lab[:, hs, wsl, :] = cnt
                cnt += 1
        mw = _windows(lab, ws).squeeze(-1)
        d = mw.unsqueeze(1) - mw.unsqueeze(2)
        mask = torch.where(d != 0, torch.full_like(d, -100.0), torch.zeros_like(d))
    win = _windows(x, ws)
    nW_, N, _ = win.shape
    hd = C // heads
    qkv = F.linear(win, sd[p + "w_msa.qkv.weight"], sd.get(p + "w_msa.qkv.bias"))
    qkv = qkv.reshape(nW_, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0] * (hd ** -0.5), qkv[1], qkv[2]
    attn = q @ k.transpose(-2, -1) + _rel_bias(sd, p + "w_msa.", heads, ws).unsqueeze(0)
    if mask is not None:
        nw = mask.shape[0]
        attn = (attn.view(-1, nw, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    attn = attn.softmax(-1)
    o = (attn @ v).transpose(1, 2).reshape(nW_, N, C)
    o = F.linear(o, sd[p + "w_msa.proj.weight"], sd[p + "w_msa.proj.bias"])
    x = _unwindows(o, B, Hp, Wp, ws)
    if shift > 0:
        x = torch.roll(x, shifts=(shift, shift), dims=(1, 2))
    return x[:, :H, :W, :].reshape(B, H * W, C)


def _ln(sd, p, x):
    return F.layer_norm(x, (x.shape[-1],), sd[p + "weight"], sd[p + "bias"], 1e-5)


def swin_block(sd, p, x, hw, heads, ws, shift):
    y = x + shift_window_msa(sd, p + "attn.", _ln(sd, p + "norm1.", x), hw, heads, ws, shift)
    h = F.gelu(F.linear(_ln(sd, p + "norm2.", y), sd[p + "ffn.layers.0.0.weight"], sd[p + "ffn.layers.0.0.bias"]))
    return y + F.linear(h, sd[p + "ffn.layers.1.weight"], sd[p + "ffn.layers.1.bias"])


def patch_embed(sd, img, patch=4):
    H, W = img.shape[-2:]
    img = F.pad(img, (0, (-W) % patch, 0, (-H) % patch))                     # AdaptivePadding 'corner'
    x = F.conv2d(img, sd["patch_embed.projection.weight"], sd["patch_embed.projection.bias"], stride=patch)
    hw = x.shape[2:]
    x = x.flatten(2).transpose(1, 2)
    return _ln(sd, "patch_embed.norm.", x), tuple(hw)


def patch_merging(sd, p, x, hw):
    B, L, C = x.shape
    H, W = hw
    x = x.view(B, H, W, C).permute(0, 3, 1, 2)
    x = F.pad(x, (0, W % 2, 0, H % 2))                                      # AdaptivePadding 'corner'
    Ho, Wo = x.shape[2] // 2, x.shape[3] // 2
    x = F.unfold(x, kernel_size=2, stride=2).transpose(1, 2)                # [B, L', C*4], c*4 + kh*2 + kw
    return F.linear(_ln(sd, p + "norm.", x), sd[p + "reduction.weight"]), (Ho, Wo)


def swin_forward(sd, img, cfg=BACKBONE):
    """SwinTransformer.forward (eval) -> list of NCHW maps for cfg['out_indices']"""
    ws = cfg["window_size"]
    x, hw = patch_embed(sd, img)
    outs = []
    C = cfg["embed_dims"]
    for i, depth in enumerate(cfg["depths"]):
        for j in range(depth):
            x = swin_block(sd, f"stages.{i}.blocks.{j}.", x, hw, cfg["num_heads"][i], ws, ws // 2 if j % 2 else 0)
        if i in cfg["out_indices"]:
            o = _ln(sd, f"norm{i}.", x)
            outs.append(o.view(-1, hw[0], hw[1], C).permute(0, 3, 1, 2).contiguous())
        if i < len(cfg["depths"]) - 1:
            x, hw = patch_merging(sd, f"stages.{i}.downsample.", x, hw)
            C *= 2
    return outs


def _conv_module(sd, p, x, padding):
    x = F.conv2d(x, sd[p + "conv.weight"], sd.get(p + "conv.bias"), padding=padding)
    x = F.batch_norm(x, sd[p + "bn.running_mean"], sd[p + "bn.running_var"], sd[p + "bn.weight"], sd[p + "bn.bias"],
                     False, 0.0, 1e-5)
    return F.relu(x)


def neck_forward(sd, feats):
    """GeneralizedLSSFPN.forward (eval, start_level 0) -> tuple of the finer len(feats) - 1 maps"""
    lat = list(feats)
    for i in range(len(lat) - 2, -1, -1):
        up = F.interpolate(lat[i + 1], size=lat[i].shape[2:], mode="bilinear", align_corners=True)
        x = torch.cat([lat[i], up], 1)
        x = _conv_module(sd, f"lateral_convs.{i}.", x, 0)
        lat[i] = _conv_module(sd, f"fpn_convs.{i}.", x, 1)
    return tuple(lat[:-1])


def cast(sd, dtype, device="cpu"):
    return {k: (v.to(device=device, dtype=dtype) if v.dtype.is_floating_point else v.to(device))
            for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------- golden samples
def sample_index(seed, numel, count=4096):
    return np.random.RandomState(seed).randint(0, numel, size=min(count, numel))


def summarize(name, t, seed, out):
    """a seeded element sample and the per-channel sums of an NCHW map, in float64"""
    a = t.detach().double().cpu().numpy()
    idx = sample_index(seed, a.size)
    out[name + "_sample"] = a.reshape(-1)[idx]
    out[name + "_chsum"] = a.sum(axis=(0, 2, 3))
    out[name + "_shape"] = np.array(a.shape, np.int64)
