"""GPU tests of the camera input pre-pass (isf_image.hip through input_pipeline.MultiViewImageLoader) against
tests/golden/image_ref.npz: what the reference's ImageAug3D + ImageNormalize give with the real Pillow, bit for bit.
Goldens only: no reference tree, no Pillow."""
import os

import numpy as np
import pytest
import torch

import image_common as ic
from isfusion_amd import input_pipeline as ip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "image_ref.npz"))


def _loader(name, **over):
    case = ic.CASES[name]
    return ip.MultiViewImageLoader(final_dim=case["final_dim"], mean=ic.MEAN, std=ic.STD, device=DEV,
                                   **dict(case["loader"], **over))


def _case(name, ref):
    """(results_list, per-sample draws) of a golden case"""
    imgs = ic.case_images(name)
    draws = ic.unpack_draws(ref[name + "_draws"], ic.CASES[name]["final_dim"])
    per_sample, at = [], 0
    for sample in imgs:
        per_sample.append(draws[at:at + len(sample)])
        at += len(sample)
    return [dict(img=sample) for sample in imgs], per_sample


def _run_on_nan(loader, results, draws):
    fH, fW = loader.final_dim
    views = sum(len(r["img"]) for r in results)
    out = torch.full((views, 3, fH, fW), float("nan"), dtype=torch.float32, device=DEV)
    img, mats = loader(results, aug=draws, out=out)
    assert img.data_ptr() == out.data_ptr() and img.shape == (len(results), len(results[0]["img"]), 3, fH, fW)
    return img.view(views, 3, fH, fW).cpu().numpy(), mats


# 5 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small_train", "small_fixed", "small_shrink"])
def test_small_cases_equal_pillow_bit_for_bit(ref, name):
    loader = _loader(name)
    results, draws = _case(name, ref)
    got, mats = _run_on_nan(loader, results, draws)
    lut, want = loader._lut, ref[name + "_u8"]
    for v in range(len(want)):
        u8 = ic.to_u8(got[v], lut)            # fails on NaN (an element not written) or any value outside the table
        bad = int((u8 != want[v]).sum())
        assert bad == 0, f"view {v}: {bad} of {want[v].size} bytes differ from Pillow"
    assert np.array_equal(got[0], ref[name + "_f32_view0"])
    assert np.array_equal(mats.numpy().reshape(-1, 4, 4), ref[name + "_aug_matrix"])


def test_full_size_cases_equal_pillow_bit_for_bit(ref):
    loader = _loader("full")
    results, draws = _case("full", ref)
    got, mats = _run_on_nan(loader, results, draws)
    for v in range(got.shape[0]):
        u8 = ic.to_u8(got[v], loader._lut)
        crc, sums = ic.summarize(u8)
        assert np.array_equal(u8.reshape(-1)[ic.sample_positions(v, u8.size)], ref["full_samples"][v]), v
        assert np.array_equal(sums, ref["full_sums"][v]), v
        assert crc == int(ref["full_crc"][v]), v
        assert np.array_equal(got[v].reshape(-1)[ic.sample_positions(v, got[v].size)], ref["full_f32_samples"][v]), v
    assert np.array_equal(mats.numpy().reshape(-1, 4, 4), ref["full_aug_matrix"])


# 6 ------------------------------------------------------------------------------------------------------------------
def test_batch_call_equals_per_sample_calls(ref):
    loader = _loader("small_fixed")
    results, draws = _case("small_fixed", ref)
    assert len({im.shape for r in results for im in r["img"]}) > 1        # mixed source sizes in one batch
    whole, mats = loader(results, aug=draws)
    for b in range(len(results)):
        one, m1 = loader([results[b]], aug=[draws[b]])
        assert torch.equal(one[0], whole[b]) and torch.equal(m1[0], mats[b])


# 7 ------------------------------------------------------------------------------------------------------------------
def test_loader_makes_no_host_sync_and_is_deterministic(ref):
    loader = _loader("small_train")
    results, draws = _case("small_train", ref)
    first, _ = loader(results, aug=draws)          # pins the staging buffers
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second, _ = loader(results, aug=draws)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(first, second)
    np.random.seed(5)
    a, ma = loader(results)                        # draws of its own
    np.random.seed(5)
    b, mb = loader(results)
    assert torch.equal(a, b) and torch.equal(ma, mb) and not torch.equal(a, first)


# 8 ------------------------------------------------------------------------------------------------------------------
def test_loader_output_feeds_the_detector(ref):
    """plumbing only: (img, img_aug_matrix) of the test-time loader at full size go through simple_test"""
    from test_gpu_camera import _detector
    det, (pts, _, kw, metas) = _detector()
    loader = _loader("full", **ic.TEST)
    results = [dict(img=[ic.image(300 + 6 * b + v, 900, 1600) for v in range(6)]) for b in range(len(pts))]
    img, mats = loader(results)
    assert img.shape == (len(pts), 6, 3, 384, 1056) and mats.shape == (len(pts), 6, 4, 4)
    assert np.array_equal(mats[0, 0].numpy(), ref["full_aug_matrix"][0])
    u8 = ic.to_u8(img[0, 0].cpu().numpy(), loader._lut)                   # sample 0, view 0 is the golden's first view
    assert ic.summarize(u8)[0] == int(ref["full_crc"][0])
    out = det.simple_test(pts, [dict(m) for m in metas], img=img, **dict(kw, img_aug_matrix=mats))
    assert len(out) == len(pts)
    for r in out:
        boxes = r["pts_bbox"]["boxes_3d"]
        boxes = boxes.tensor if hasattr(boxes, "tensor") else boxes
        assert boxes.shape[0] > 0 and torch.isfinite(boxes).all() and torch.isfinite(r["pts_bbox"]["scores_3d"]).all()
