"""CPU tests of the camera backbone's mixed-precision training mode (SwinTransformer.set_precision("mixed"),
ISFusionDetector.camera_precision): the attribute surface, the unchanged state dict, the C symbols of the mode, and the
conditioning guards of the GPU comparisons (tests/test_gpu_camera_mixed.py), recomputed here under
torch.autocast("cpu", float16): err_autocast <= 1e-2 * max|ref| for maps and attention gradients, 2e-2 for parameter
gradients, for every backbone and attention case the GPU tests use."""
import ctypes
import os
import re

import pytest
import torch

import camera_mixed_common as CM
import camera_train_common as CT
from test_camera import _model, _modules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED_SYMBOLS = ("isf_swin_gemm_f16_rowscale", "isf_rows_weight_grad_f16", "isf_swin_window_attention_backward_f16")
# parameter counts the mode must not move
OLD_COUNTS = {"isf_swin_gemm": 13, "isf_swin_gemm_rowscale": 15, "isf_swin_gemm_f16": 15, "isf_rows_weight_grad": 13,
              "isf_swin_window_attention_backward": 22, "isf_swin_window_attention_f16": 13, "isf_pack_linear_f16": 5}


def test_mixed_mode_surface():
    from isfusion_amd import registry
    bb, _ = _modules()
    assert "mixed" in bb.PRECISIONS and bb.PRECISIONS[:2] == ("f32", "f16")
    keys = list(bb.state_dict())
    assert bb.set_precision("mixed") is bb and bb.precision == "mixed"
    assert list(bb.state_dict()) == keys and len(keys) == 187
    assert "precision" not in dict(bb.named_buffers()) and "precision" not in dict(bb.named_parameters())
    bb.train()
    bb.set_precision("f16")
    with pytest.raises(NotImplementedError, match="f16"):          # "f16" stays an inference mode
        bb.forward_train(torch.zeros(1, 3, 32, 32))
    bb.set_precision("mixed")
    with pytest.raises(Exception) as info:                         # accepted: it gets as far as asking for the device
        bb.forward_train(torch.zeros(1, 3, 32, 32))
    assert not isinstance(info.value, NotImplementedError) and "GPU" in str(info.value)
    bb.drop_rate = 0.1
    with pytest.raises(NotImplementedError, match="drop_rate"):
        bb.forward_train(torch.zeros(1, 3, 32, 32))
    det = registry.build_detector({"model": _model()})
    det.camera_precision = "mixed"
    assert det.img_backbone.precision == "mixed" and det.camera_precision == "mixed"
    det.camera_precision = "f32"
    assert det.img_backbone.precision == "f32"
    assert "precision" not in " ".join(det.state_dict())


def test_mixed_symbols_declared_bound_and_exported():
    from isfusion_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "isf_hip.h")) as f:
        hdr = f.read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)

    def declared_params(name):
        return len(re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S).group(1).split(","))

    for name in MIXED_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert declared_params(name) == len(_lib.SIGNATURES[name][1]), name
    for name, count in OLD_COUNTS.items():
        assert declared_params(name) == len(_lib.SIGNATURES[name][1]) == count, name
    # the new entries add their own parameters to the ones they extend, and nothing else
    assert declared_params("isf_swin_gemm_f16_rowscale") == OLD_COUNTS["isf_swin_gemm_f16"] + 2
    assert declared_params("isf_rows_weight_grad_f16") == OLD_COUNTS["isf_rows_weight_grad"]
    assert declared_params("isf_swin_window_attention_backward_f16") == OLD_COUNTS["isf_swin_window_attention_backward"]
    # a section of their own, after the fp32 backward's block, citing the reference lines they replace
    block = hdr[hdr.index("Mixed-precision training of the Swin-T backbone"):]
    assert hdr.index("Mixed-precision training of the Swin-T backbone") > hdr.index("int isf_swin_operand_rows")
    for name in MIXED_SYMBOLS:
        entry = block[block.index(" * " + name):]
        entry = entry[:re.search(r"\n \* isf_|\*/", entry[3:]).start() + 3]
        assert re.search(r"swin\.py:\d+|mmcv FFN", entry), name


def test_no_float_atomics_in_the_mixed_backward():
    src = open(os.path.join(ROOT, "is-fusion_amd", "csrc", "isf_swin_train_f16.hip")).read()
    assert not re.search(r"atomic", src, flags=re.I)
    assert "isf_swin_train_f16.hip" in open(os.path.join(ROOT, "is-fusion_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("case", range(len(CM.ATTENTION) + 1))
def test_attention_guards_under_cpu_autocast(case):
    """every attention case of the GPU test, and the large-|v| case last"""
    wide = case == len(CM.ATTENTION)
    case = CM.RANGE_CASE if wide else case
    B, H, W, heads, shift = CM.ATTENTION[case]
    t = CM.attention_inputs(case, CM.V_BOUND if wide else None)
    ref, ac = CM.attention_yardsticks(case, t, "cpu")
    tag = f"attention {CM.ATTENTION[case]}" + (" |v| <= 32" if wide else "")
    CM.guard(f"{tag} out", ac[0], ref[0], CM.GUARD_ROWS)
    CM.guard(f"{tag} dqkv", ac[1], ref[1], CM.GUARD_ROWS)
    CM.guard(f"{tag} dqkv_bias", ac[2], ref[2], CM.GUARD_PARAMS)
    CM.guard(f"{tag} dtable", ac[3], ref[3], CM.GUARD_PARAMS)
    C = 32 * heads
    assert bool((ref[2][:C] == 0).all())
    if H % 7 == 0 and W % 7 == 0:
        assert bool((ref[2] == 0).all()) and bool((ac[2] == 0).all())      # exactly zero: the GPU test asks the same
    else:
        assert float(ref[2][C:].abs().max()) > 1e-2


@pytest.mark.parametrize("size", CT.TRAIN_SIZES)
def test_backbone_guards_under_cpu_autocast(size):
    sd, img, keep = CM.backbone_inputs(size)
    o64, g64 = CM.backbone_yardstick(sd, img, keep, None, torch.float64, "cpu")
    oac, gac = CM.backbone_yardstick(sd, img, keep, None, torch.float32, "cpu")
    for i, (a, r) in enumerate(zip(oac, o64)):
        CM.guard(f"backbone {size} map {i}", a, r, CM.GUARD_ROWS)
    assert sorted(g64) == sorted(gac) and len(g64) == 187 - 12        # the relative_position_index buffers
    worst = max((CM.guard(f"backbone {size} grad {k}", gac[k], g64[k], CM.GUARD_PARAMS), k) for k in sorted(g64))
    print(f"backbone {size}: worst parameter-gradient err_autocast / max|ref| {worst[0]:.3e} ({worst[1]})")
