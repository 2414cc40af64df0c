"""CPU tests of the camera backbone's f16 inference mode (SwinTransformer.set_precision,
ISFusionDetector.camera_precision): the attribute surface, the unchanged state dict, the training-mode refusal and the
C symbols of the mode.  Also the conditioning guard of the GPU comparisons (tests/test_gpu_camera_f16.py): the float64
restatement under CPU autocast(float16) stays within 1e-2 of the float64 result for the seeds those tests use."""
import ctypes
import os
import re

import pytest
import torch

import camera_common as CC
from test_camera import BACKBONE_SEED, _model, _modules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16_SYMBOLS = ("isf_swin_gemm_f16", "isf_swin_window_attention_f16", "isf_pack_linear_f16",
               "isf_packed_linear_f16_bytes")
# (images, H, W, image seed) of the whole-backbone comparisons on the GPU: the golden sizes
BACKBONE_CASES = ((3, 90, 150, 101), (2, 128, 352, 100))


def test_precision_attribute_surface():
    from isfusion_amd import registry
    bb, _ = _modules()
    assert bb.precision == "f32"
    assert bb.set_precision("f16") is bb and bb.precision == "f16"
    bb.set_precision("f32")
    assert bb.precision == "f32"
    with pytest.raises(ValueError, match="bf16"):
        bb.set_precision("bf16")
    assert bb.precision == "f32"
    det = registry.build_detector({"model": _model()})          # the unmodified reference config still builds
    assert det.camera_precision == "f32" and det.img_backbone.precision == "f32"
    det.camera_precision = "f16"
    assert det.img_backbone.precision == "f16" and det.camera_precision == "f16"
    det.img_backbone.set_precision("f32")
    assert det.camera_precision == "f32"
    with pytest.raises(ValueError):
        det.camera_precision = "fp8"


def test_state_dict_is_unchanged_by_the_mode():
    bb, _ = _modules()
    keys = list(bb.state_dict())
    bb.set_precision("f16")
    assert list(bb.state_dict()) == keys and len(keys) == 187
    assert "precision" not in dict(bb.named_buffers()) and "precision" not in dict(bb.named_parameters())
    bb.load_state_dict(CC.seeded_module_state(bb, BACKBONE_SEED), strict=True)
    assert bb.precision == "f16"


def test_forward_train_refuses_the_f16_mode_before_touching_the_device():
    bb, _ = _modules()
    bb.train()
    bb.set_precision("f16")
    with pytest.raises(NotImplementedError, match="f16"):
        bb.forward_train(torch.zeros(1, 3, 32, 32))


def test_f16_symbols_declared_mirrored_and_exported():
    from isfusion_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "isf_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in F16_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # the entry points of the default mode keep their signatures
    assert len(_lib.SIGNATURES["isf_swin_gemm"][1]) == 13 and len(_lib.SIGNATURES["isf_swin_window_attention"][1]) == 13


@pytest.mark.parametrize("case", range(len(BACKBONE_CASES)))
def test_guard_inputs_are_well_conditioned_under_cpu_autocast(case):
    """the guard of the GPU comparisons, shown without a GPU: err_autocast <= 1e-2 * max|ref| for every out_indices map"""
    n, h, w, seed = BACKBONE_CASES[case]
    bb, _ = _modules()
    sd = CC.seeded_module_state(bb, BACKBONE_SEED)
    img = CC.images(seed, n, h, w)
    with torch.no_grad():
        ref = CC.swin_forward(CC.cast(sd, torch.float64), img.double())
        with torch.autocast("cpu", dtype=torch.float16):
            ac = CC.swin_forward(CC.cast(sd, torch.float32), img)
    for a, r in zip(ac, ref):
        err, top = float((a.double() - r).abs().max()), float(r.abs().max())
        print(f"case {case}: err_autocast {err:.3e}, max|ref| {top:.3e}")
        assert err <= 1e-2 * top, (err, top)
