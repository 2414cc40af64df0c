"""Training-mode float64 restatement of the camera branch: tests/camera_common.py's SwinTransformer with stochastic
depth (DropPath masks given by the caller) and GeneralizedLSSFPN with batch-statistics BatchNorm.  Gradients come from
autograd over it.  tests/test_camera_train.py pins it to tests/golden/camera_train_ref.npz (the reference's own modules
in training mode); the GPU tests use it as the yardstick.

DropPath is mmcv's definition: per image keep = floor(keep_prob + U[0, 1)), branch output * keep / keep_prob; the
restatement takes `keep` (0 / 1 per drawing layer and image) as an argument.  Drawing layers: by block, the attention
branch before the FFN; a block whose rate is 0 draws nothing."""
import numpy as np
import torch
import torch.nn.functional as F

import camera_common as CC

TRAIN_SIZES = ((3, 90, 150), (2, 64, 160))   # (images, H, W): odd stage grids (merge + patch padding) / even grids


def drop_path_rates(cfg=CC.BACKBONE):
    """per-block rates: linspace(0, drop_path_rate, number of blocks), computed as the module does (float32 linspace)"""
    return [x.item() for x in torch.linspace(0, cfg["drop_path_rate"], sum(cfg["depths"]))]


def drop_layers(cfg=CC.BACKBONE):
    """rates of the layers that draw a mask, in mask-row order"""
    return [r for r in drop_path_rates(cfg) for _ in range(2) if r > 0.0]


def fixed_drop_keep(seed, n, cfg=CC.BACKBONE):
    """[len(drop_layers), n] of 0 / 1 with, in EVERY layer, at least one image dropped and one kept (n >= 2)"""
    rng = np.random.RandomState(seed)
    L = len(drop_layers(cfg))
    keep = (rng.uniform(size=(L, n)) < 0.6).astype(np.float32)
    for i in range(L):
        keep[i, i % n] = 0.0
        keep[i, (i + 1) % n] = 1.0
    return torch.from_numpy(keep)


def swin_block_train(sd, p, x, hw, heads, ws, shift, s_attn, s_ffn):
    """SwinBlock in training mode: x + drop(attn(norm1 x)); then identity + drop(ffn layers(norm2 .)).  s_*: [B] factors
    keep / keep_prob or None (rate 0)"""
    a = CC.shift_window_msa(sd, p + "attn.", CC._ln(sd, p + "norm1.", x), hw, heads, ws, shift)
    if s_attn is not None:
        a = a * s_attn.view(-1, 1, 1)
    y = x + a
    h = F.gelu(F.linear(CC._ln(sd, p + "norm2.", y), sd[p + "ffn.layers.0.0.weight"], sd[p + "ffn.layers.0.0.bias"]))
    f = F.linear(h, sd[p + "ffn.layers.1.weight"], sd[p + "ffn.layers.1.bias"])
    if s_ffn is not None:
        f = f * s_ffn.view(-1, 1, 1)
    return y + f


def swin_forward_train(sd, img, keep, cfg=CC.BACKBONE):
    """SwinTransformer.forward in training mode with the DropPath masks keep [len(drop_layers), N] -> NCHW maps"""
    ws = cfg["window_size"]
    rates = drop_path_rates(cfg)
    x, hw = CC.patch_embed(sd, img)
    outs = []
    C = cfg["embed_dims"]
    blk = row = 0
    for i, depth in enumerate(cfg["depths"]):
        for j in range(depth):
            sa = sf = None
            if rates[blk] > 0.0:
                kp = 1.0 - rates[blk]
                sa, sf = keep[row].to(x.dtype) / kp, keep[row + 1].to(x.dtype) / kp
                row += 2
            x = swin_block_train(sd, f"stages.{i}.blocks.{j}.", x, hw, cfg["num_heads"][i], ws, ws // 2 if j % 2 else 0,
                                 sa, sf)
            blk += 1
        if i in cfg["out_indices"]:
            o = CC._ln(sd, f"norm{i}.", x)
            outs.append(o.view(-1, hw[0], hw[1], C).permute(0, 3, 1, 2).contiguous())
        if i < len(cfg["depths"]) - 1:
            x, hw = CC.patch_merging(sd, f"stages.{i}.downsample.", x, hw)
            C *= 2
    assert row == len(drop_layers(cfg))
    return outs


def _conv_module_train(sd, p, x, padding, momentum=0.1):
    """ConvModule in training mode: conv -> BatchNorm2d with batch statistics (eps 1e-5; sd's running_mean /
    running_var are updated in place, num_batches_tracked + 1) -> ReLU"""
    x = F.conv2d(x, sd[p + "conv.weight"], None, padding=padding)
    x = F.batch_norm(x, sd[p + "bn.running_mean"], sd[p + "bn.running_var"], sd[p + "bn.weight"], sd[p + "bn.bias"],
                     True, momentum, 1e-5)
    sd[p + "bn.num_batches_tracked"] = sd[p + "bn.num_batches_tracked"] + 1
    return F.relu(x)


def neck_forward_train(sd, feats):
    """GeneralizedLSSFPN.forward in training mode -> tuple of the finer len(feats) - 1 maps; sd's BatchNorm buffers move"""
    lat = list(feats)
    for i in range(len(lat) - 2, -1, -1):
        up = F.interpolate(lat[i + 1], size=lat[i].shape[2:], mode="bilinear", align_corners=True)
        x = torch.cat([lat[i], up], 1)
        x = _conv_module_train(sd, f"lateral_convs.{i}.", x, 0)
        lat[i] = _conv_module_train(sd, f"fpn_convs.{i}.", x, 1)
    return tuple(lat[:-1])


def leaf_params(sd, dtype, device="cpu"):
    """a copy of sd in which every floating non-buffer entry is a leaf that requires grad"""
    out = {}
    for k, v in sd.items():
        if not v.dtype.is_floating_point:
            out[k] = v.clone().to(device)
        elif k.endswith(("running_mean", "running_var")):
            out[k] = v.detach().clone().to(device=device, dtype=dtype)
        else:
            out[k] = v.detach().clone().to(device=device, dtype=dtype).requires_grad_(True)
    return out


def upstream(seed, shape, dtype=torch.float64):
    """a seeded upstream gradient"""
    return torch.from_numpy(np.random.RandomState(seed).normal(0.0, 1.0, tuple(shape))).to(dtype)
