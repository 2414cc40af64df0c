"""CPU tests of the camera branch (SwinTransformer, GeneralizedLSSFPN, ISFusionDetector): the float64 restatement
against the reference's own outputs (tests/golden/camera_ref.npz), the state-dict surface, the config builder, the
options that must raise, and the C symbols of isf_swin.hip."""
import ast
import ctypes
import os

import numpy as np
import pytest
import torch

import camera_common as CC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "camera_ref.npz")
BACKBONE_SEED, NECK_SEED = 4101, 4202      # tests/golden/make_golden_camera.py


def _golden():
    return np.load(GOLDEN, allow_pickle=False)


def _model():
    with open(os.path.join(HERE, "golden", "isfusion_0075voxel_model.txt")) as f:
        return ast.literal_eval(f.read())


def _modules():
    from isfusion_amd.generalized_lss import GeneralizedLSSFPN
    from isfusion_amd.swin import SwinTransformer
    m = _model()
    bb, nk = dict(m["img_backbone"]), dict(m["img_neck"])
    bb.pop("type"), nk.pop("type")
    return SwinTransformer(**bb), GeneralizedLSSFPN(**nk)


def check_summary(g, name, t, seed, rtol, atol):
    a = t.detach().double().cpu().numpy()
    assert tuple(a.shape) == tuple(g[name + "_shape"]), (name, a.shape)
    idx = CC.sample_index(seed, a.size)
    np.testing.assert_allclose(a.reshape(-1)[idx], g[name + "_sample"], rtol=rtol, atol=atol, err_msg=name)
    ch = a.sum(axis=(0, 2, 3))
    scale = np.abs(a).sum(axis=(0, 2, 3)) + 1.0
    assert np.all(np.abs(ch - g[name + "_chsum"]) <= rtol * scale + atol), name


@pytest.mark.parametrize("case", range(len(CC.GOLDEN_SIZES)))
def test_restatement_reproduces_reference(case):
    g = _golden()
    bb, nk = _modules()
    sdb = CC.cast(CC.seeded_module_state(bb, BACKBONE_SEED), torch.float64)
    sdn = CC.cast(CC.seeded_module_state(nk, NECK_SEED), torch.float64)
    n, h, w = CC.GOLDEN_SIZES[case]
    img = CC.images(100 + case, n, h, w).double()
    feats = CC.swin_forward(sdb, img)
    necks = CC.neck_forward(sdn, feats)
    assert len(feats) == 3 and len(necks) == 2
    for li, t in enumerate(feats):
        check_summary(g, f"c{case}_bb{li}", t, 10 * case + li, 1e-9, 1e-9)
    for li, t in enumerate(necks):
        check_summary(g, f"c{case}_neck{li}", t, 10 * case + 5 + li, 1e-9, 1e-9)


def test_state_dict_matches_reference_keys():
    g = _golden()
    bb, nk = _modules()
    keys = ["img_backbone." + k for k in bb.state_dict()] + ["img_neck." + k for k in nk.state_dict()]
    shapes = [",".join(str(s) for s in v.shape) for v in list(bb.state_dict().values()) + list(nk.state_dict().values())]
    assert keys == list(g["keys"])
    assert shapes == list(g["key_shapes"])
    assert len(bb.state_dict()) == 187
    assert sum(p.numel() for p in bb.parameters()) == int(g["backbone_params"])
    sd = bb.state_dict()
    assert "stages.0.blocks.0.ffn.layers.0.0.weight" in sd and "stages.3.blocks.1.ffn.layers.1.bias" in sd
    assert sd["stages.0.blocks.0.attn.w_msa.relative_position_index"].dtype == torch.int64
    # the golden weights load strictly, relative_position_index included
    bb.load_state_dict(CC.seeded_module_state(bb, BACKBONE_SEED), strict=True)


def test_build_detector_from_config():
    from isfusion_amd import registry
    from isfusion_amd.detector import ISFusionDetector, ISFusionPtsPath
    from isfusion_amd.generalized_lss import GeneralizedLSSFPN
    from isfusion_amd.swin import SwinTransformer
    model = _model()
    det = registry.build_detector({"model": model})
    assert isinstance(det, ISFusionDetector) and isinstance(det, ISFusionPtsPath)
    assert isinstance(det.img_backbone, SwinTransformer) and isinstance(det.img_neck, GeneralizedLSSFPN)
    assert det.detach is True and det.img_backbone.out_indices == [1, 2, 3]
    det2 = registry.build_detector(model)
    assert list(det2.state_dict()) == list(det.state_dict())
    pts = registry.build_pts_path({"model": model})
    keys = set(det.state_dict())
    cam = {k for k in keys if k.startswith(("img_backbone.", "img_neck."))}
    assert keys - cam == set(pts.state_dict())
    assert sorted(cam) == sorted(_golden()["keys"])
    assert registry.lookup("SwinTransformer") is SwinTransformer
    assert registry.lookup("GeneralizedLSSFPN") is GeneralizedLSSFPN
    assert registry.MODULES["BACKBONES"]["SwinTransformer"] is SwinTransformer
    assert registry.MODULES["NECKS"]["GeneralizedLSSFPN"] is GeneralizedLSSFPN


@pytest.mark.parametrize("kw", [dict(use_abs_pos_embed=True), dict(with_cp=True), dict(frozen_stages=0),
                                dict(convert_weights=True), dict(norm_cfg=dict(type="BN")),
                                dict(pretrained="swin.pth"), dict(window_size=12)])
def test_backbone_unsupported_options_raise(kw):
    from isfusion_amd.swin import SwinTransformer
    with pytest.raises(NotImplementedError):
        SwinTransformer(**kw)


@pytest.mark.parametrize("kw", [dict(start_level=1), dict(end_level=2), dict(conv_cfg=dict(type="Conv2d")),
                                dict(norm_cfg=dict(type="GN", num_groups=8)),
                                dict(upsample_cfg=dict(mode="nearest"))])
def test_neck_unsupported_options_raise(kw):
    from isfusion_amd.generalized_lss import GeneralizedLSSFPN
    with pytest.raises(NotImplementedError):
        GeneralizedLSSFPN([192, 384, 768], 256, 3, **kw)


def test_training_forward_raises():
    bb, nk = _modules()
    with pytest.raises(NotImplementedError, match="eval"):
        bb.train()(torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError, match="eval"):
        nk.train()([torch.zeros(1, 192, 8, 8), torch.zeros(1, 384, 4, 4), torch.zeros(1, 768, 2, 2)])


def test_new_symbols_exported():
    from isfusion_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("isf_swin_gemm", "isf_swin_row_stats", "isf_swin_layernorm", "isf_swin_window_attention"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "isf_hip.h")) as f:
        header = f.read()
    assert "int isf_swin_gemm(" in header and "typedef struct isf_swin_a" in header
