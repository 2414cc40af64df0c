"""What the CPU and GPU tests of the camera backbone's mixed-precision training mode share (tests/test_camera_mixed.py,
tests/test_gpu_camera_mixed.py): the attention cases and their inputs, the whole-backbone inputs, and the two yardsticks
of the rule

    err_hip <= 2 * err_autocast + 2^-11 * max|ref|          (err = max |x - ref64|)

-- the float64 restatement with autograd over it, and the same restatement with fp32 leaves under
torch.autocast(float16), forward and backward, on the device the caller names.  The guard keeps a comparison from passing
on ill-conditioned inputs: err_autocast <= 1e-2 * max|ref| for maps, attention outputs and input gradients, 2e-2 for
parameter gradients."""
import torch

import camera_common as CC
import camera_train_common as CT
from test_camera import BACKBONE_SEED
from test_gpu_swin_backward import ATTENTION as _F32_ATTENTION, _attention_core

U16 = 2.0 ** -11
GUARD_ROWS, GUARD_PARAMS = 1e-2, 2e-2
ATTENTION = list(_F32_ATTENTION) + [(1, 9, 10, 24, 3)]       # (B, H, W, heads, shift); the last: C = 768
V_BOUND = 32.0          # include/isf_hip.h: no f16 operand of the attention backward saturates for |v| <= 32, |dout| < 2^10
RANGE_CASE = 2          # the attention case run again with |v| up to V_BOUND


def rule(what, got, ref, ac, guard):
    """the rule and its guard; prints the figures before it asserts"""
    ref = ref.double()
    e_hip, e_ac = float((got.double() - ref).abs().max()), float((ac.double() - ref).abs().max())
    top = float(ref.abs().max())
    bound = 2 * e_ac + U16 * top
    print(f"{what}: err_hip {e_hip:.3e}  err_autocast {e_ac:.3e}  bound {bound:.3e}  max|ref| {top:.3e}")
    assert e_ac <= guard * top, (what, e_ac, top)
    assert e_hip <= bound, (what, e_hip, bound)


def guard(what, ac, ref, limit):
    """the guard alone (the CPU tests); returns err_autocast / max|ref|"""
    ref = ref.double()
    e_ac, top = float((ac.double() - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: err_autocast {e_ac:.3e}  max|ref| {top:.3e}")
    assert e_ac <= limit * top, (what, e_ac, top)
    return e_ac / top if top else 0.0


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


def attention_inputs(case, v_max=None):
    """CPU tensors: f16 qkv rows, fp32 bias (s = 0.3) and table (s = 0.5), an f16-representable unit-scale upstream, the
    relative position index.  v_max: the value third of qkv is scaled so that its largest entry is v_max."""
    from isfusion_amd.swin import WindowMSA
    B, H, W, heads, shift = ATTENTION[case]
    C = 32 * heads
    gen = torch.Generator(device="cpu")
    gen.manual_seed(5000 + case)
    qkv = _randn(gen, B * H * W, 3 * C)
    if v_max is not None:
        qkv[:, 2 * C:] *= v_max / float(qkv[:, 2 * C:].abs().max())
    return dict(qkv=qkv.half(), bias=(_randn(gen, 3 * C) * 0.3).float(), table=(_randn(gen, 169, heads) * 0.5).float(),
                up=_randn(gen, B * H * W, C).half(), index=WindowMSA(C, heads, (7, 7)).relative_position_index)


def attention_yardsticks(case, t, device):
    """(float64, autocast) -> each (out, dqkv, dbias, dtable) of _attention_core for the unit-scale upstream"""
    B, H, W, heads, shift = ATTENTION[case]
    index = t["index"].to(device)
    res = []
    for dtype in (torch.float64, torch.float32):
        leaves = [t[k].to(device=device, dtype=dtype).requires_grad_(True) for k in ("qkv", "bias", "table")]
        with torch.autocast(device, dtype=torch.float16, enabled=dtype == torch.float32):
            out = _attention_core(*leaves, index, B, H, W, heads, shift)
        grads = torch.autograd.grad(out, leaves, t["up"].to(device=device, dtype=out.dtype))
        res.append((out.detach(),) + tuple(grads))
    return res


def backbone_inputs(size):
    """(state dict, images seed 31, DropPath keep, upstream shapes -> upstreams) of the whole-backbone comparison"""
    from test_camera import _modules
    n, h, w = size
    bb, _ = _modules()
    return CC.seeded_module_state(bb, BACKBONE_SEED), CC.images(31, n, h, w), CT.fixed_drop_keep(32, n)


def upstreams(shapes):
    return [CT.upstream(700 + i, s) / float(torch.tensor(s).prod()) ** 0.5 for i, s in enumerate(shapes)]


def backbone_yardstick(sd, img, keep, ups, dtype, device):
    """maps and {name: gradient} of the training-mode restatement: float64, or fp32 leaves under autocast(float16)"""
    p = CT.leaf_params(sd, dtype, device)
    keep = keep.to(device)
    with torch.autocast(device, dtype=torch.float16, enabled=dtype == torch.float32):
        outs = CT.swin_forward_train(p, img.to(device=device, dtype=dtype), keep)
    if ups is None:
        ups = upstreams([tuple(o.shape) for o in outs])
    sum((o.to(dtype) * u.to(device=device, dtype=dtype)).sum() for o, u in zip(outs, ups)).backward()
    return [o.detach() for o in outs], {k: v.grad for k, v in p.items() if v.requires_grad}
