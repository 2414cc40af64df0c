"""CPU tests of the camera branch's training path: the float64 training-mode restatement (tests/camera_train_common.py)
against the reference's own modules in training mode (tests/golden/camera_train_ref.npz), the drop-path schedule and
mask order, the entry points that must raise, and the C symbols of the training kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import camera_common as CC
import camera_train_common as CT
from test_camera import BACKBONE_SEED, NECK_SEED, _modules, check_summary

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "camera_train_ref.npz")


def _zero_counters(sd):
    return {k: (torch.zeros_like(v) if k.endswith("num_batches_tracked") else v) for k, v in sd.items()}


@pytest.mark.parametrize("case", range(len(CT.TRAIN_SIZES)))
def test_training_restatement_reproduces_reference(case):
    """pins WHERE the drop is applied (the masks drop and keep an image in every drawing layer) and the neck's
    batch-statistics BatchNorm with its running-statistics update"""
    g = np.load(GOLDEN, allow_pickle=False)
    bb, nk = _modules()
    sdb = CC.cast(CC.seeded_module_state(bb, BACKBONE_SEED), torch.float64)
    sdn = _zero_counters(CC.cast(CC.seeded_module_state(nk, NECK_SEED), torch.float64))
    n, h, w = CT.TRAIN_SIZES[case]
    keep = CT.fixed_drop_keep(300 + case, n)
    assert all(0.0 in row and 1.0 in row for row in keep.tolist())
    img = CC.images(200 + case, n, h, w).double()
    with torch.no_grad():
        feats = CT.swin_forward_train(sdb, img, keep)
        necks = CT.neck_forward_train(sdn, feats)
        # the masks matter: the eval restatement is far away
        assert float((CC.swin_forward(sdb, img)[0] - feats[0]).abs().max()) > 1e-2
    for li, t in enumerate(feats):
        check_summary(g, f"t{case}_bb{li}", t, 10 * case + li, 1e-9, 1e-9)
    for li, t in enumerate(necks):
        check_summary(g, f"t{case}_neck{li}", t, 10 * case + 5 + li, 1e-9, 1e-9)
    checked = 0
    for k, v in sdn.items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            np.testing.assert_allclose(v.double().numpy(), g[f"t{case}_{k}"], rtol=1e-9, atol=1e-12, err_msg=k)
            checked += 1
    assert checked == 12


def test_drop_path_schedule_and_mask_rows():
    """rates = linspace(0, drop_path_rate, 12) per block; block 0 (rate 0) draws nothing; two rows per drawing block,
    attention before the FFN"""
    g = np.load(GOLDEN, allow_pickle=False)
    bb, _ = _modules()
    rates = [x.item() for x in torch.linspace(0, 0.2, 12)]
    assert bb.drop_path_rates == rates == CT.drop_path_rates()
    blocks = [blk for st in bb.stages for blk in st.blocks]
    assert [blk.attn.drop_path_rate for blk in blocks] == rates
    assert [blk.ffn.drop_path_rate for blk in blocks] == rates
    layers = bb.drop_layers()
    assert len(layers) == 22 and layers == CT.drop_layers() == list(g["drop_layers"])
    assert layers == [r for r in rates[1:] for _ in range(2)]
    assert rates[0] == 0.0 and abs(rates[-1] - 0.2) < 1e-7


def test_dropout_rates_other_than_drop_path_raise():
    from isfusion_amd.swin import SwinTransformer
    for kw in (dict(drop_rate=0.1), dict(attn_drop_rate=0.1)):
        bb = SwinTransformer(depths=(1, 1), num_heads=(3, 6), out_indices=(0, 1), **kw)
        with pytest.raises(NotImplementedError, match="drop_rate"):
            bb.train().forward_train(torch.zeros(1, 3, 32, 32))


def test_forward_train_refuses_cpu_tensors():
    from isfusion_amd._lib import IsfError
    bb, nk = _modules()
    with pytest.raises(IsfError):
        bb.train().forward_train(torch.zeros(1, 3, 32, 32))
    with pytest.raises(IsfError):
        nk.train().forward_train([torch.zeros(1, 192, 8, 8), torch.zeros(1, 384, 4, 4), torch.zeros(1, 768, 2, 2)])
    # forward() in training mode keeps raising, and now names forward_train
    with pytest.raises(NotImplementedError, match="forward_train"):
        bb.train()(torch.zeros(1, 3, 32, 32))


def test_detector_training_needs_detach():
    from isfusion_amd.detector import ISFusionDetector
    import inspect
    sig = inspect.signature(ISFusionDetector.forward_train)
    assert list(sig.parameters)[1:10] == ["points", "img_metas", "gt_bboxes_3d", "gt_labels_3d", "gt_labels", "gt_bboxes",
                                          "img", "proposals", "gt_bboxes_ignore"]
    from isfusion_amd import registry
    from test_camera import _model
    det = registry.build_detector({"model": _model()})
    assert det.detach is True
    det.detach = False
    det.train()
    with pytest.raises(NotImplementedError, match="Swin"):
        det.extract_img_feat(torch.zeros(1, 1, 3, 32, 32), [dict()])


def test_training_symbols_declared_mirrored_exported():
    from isfusion_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "isf_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("isf_swin_gemm_rowscale", "isf_upsample_rows_adjoint", "isf_rows_weight_grad",
                 "isf_rows_weight_grad_chunks"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
        assert f"int {name}(" in header
    # the chunk count: whole 32-row steps per chunk, no empty chunk, about 512 workgroups over the 128 x 64 tiles
    lib = _lib.load()
    for (R, N, K), want in (((130, 256, 192), 5), ((4103, 256, 192), 65), ((4103, 64, 1152), 26),
                            ((19008, 256, 384), 43), ((1, 16, 32), 1)):
        assert lib.isf_rows_weight_grad_chunks(R, N, K) == want, (R, N, K)
