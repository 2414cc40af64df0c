"""GPU tests of the attention-probability dropout beyond 512 keys: the forward's 512-key splits + merge with the mask, the
backward's key-split route (dropout, more than 512 keys, at most 256 queries: isf_attention_bwd.hip) and the parent's
kernels on the shapes around it, against float64 softmax attention with the SAME mask (fusion_ops.attention_keep_mask); then
fusion_train._mha and the detection head with `cross_attention_dropout` against float64 compositions that apply the masks of
the seeds the calls drew (tests/head_dropout_common.py)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import head_dropout_common as H  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def rel_err(got, want):
    """max |got - want| / max(1, max |want|), the measure tests/test_gpu_train.py uses"""
    return (got.detach().cpu().double() - want.detach().double()).abs().max().item() / max(1.0, want.detach().abs().max().item())


# (B, Lq, Lk): what the case can catch
SHAPES = [
    (2, 20, 513),      # the second split holds one key: 15 masked rows in its tile
    (2, 37, 1040),     # the last split is exactly one 16-key tile; Lq no multiple of 16
    (1, 200, 1296),    # the small head's keys under the full head's queries; three splits
    (1, 256, 513),     # the last query count on the key-split backward ...
    (1, 257, 513),     # ... and the first on the parent's wave kernels
    (1, 300, 700),     # two query blocks in the forward; wave kernels with more than 512 keys
    (1, 2100, 600),    # lane kernels; key tiles 4 x 128 + 88
    (1, 16, 32400),    # 64 splits, the last of 144 keys; key indices up to 32399; workspace sizing
]


@pytest.mark.parametrize("B,Lq,Lk", SHAPES)
def test_dropout_beyond_512_keys_matches_the_masked_float64_reference(B, Lq, Lk):
    """inputs, measure and bounds of test_attention_probability_dropout_matches_the_masked_float64_reference
    (tests/test_gpu_train.py; 1e-5 on the output, 1e-4 on dq / dk / dv), p = 0.3: p = 0 is the plain call bit for bit,
    another seed another output, the keep rate within 0.01 of 1 - p, and forward + backward repeat bit for bit (every sum in a
    fixed order, no atomics).  Observed on an MI355X over the eight shapes: output at most 7.7e-7, gradients at most 9.3e-7."""
    from isfusion_amd import fusion_ops as ops
    E, nhead, p, seed = 128, 8, 0.3, 0x1234567890ABCDEF
    q, k, v = rnd((B * Lq, E), 81), rnd((B * Lk, E), 82), rnd((B * Lk, E), 83)
    w = rnd((B * Lq, E), 84)

    def run():
        qg, kg, vg = (t.to(DEV).requires_grad_() for t in (q, k, v))
        out = ops.AttentionFunction.apply(qg, kg, vg, B, Lq, Lk, E, nhead, p, seed)
        (out * w.to(DEV)).sum().backward()
        return out.detach(), qg.grad, kg.grad, vg.grad

    out, dq, dk, dv = run()
    mask = ops.attention_keep_mask(seed, B, nhead, Lq, Lk, p)                     # [B, heads, Lq, Lk]
    assert abs(mask.double().mean().item() - (1 - p)) < 0.01
    qr, kr, vr = (t.double().requires_grad_() for t in (q, k, v))
    ref = H.masked_attention(qr, kr, vr, B, Lq, Lk, nhead, mask, p)
    (ref * w.double()).sum().backward()
    errs = dict(out=rel_err(out, ref), dq=rel_err(dq, qr.grad), dk=rel_err(dk, kr.grad), dv=rel_err(dv, vr.grad))
    print("attention dropout", (B, Lq, Lk), {n: "%.2e" % e for n, e in errs.items()})
    assert errs["out"] < 1e-5, errs
    for name in ("dq", "dk", "dv"):
        assert errs[name] < 1e-4, (name, errs)
    for a, b, name in zip(run(), (out, dq, dk, dv), ("out", "dq", "dk", "dv")):
        assert torch.equal(a, b), name                                            # repeats bit for bit
    plain = ops.AttentionFunction.apply(q.to(DEV), k.to(DEV), v.to(DEV), B, Lq, Lk, E, nhead)
    assert torch.equal(ops.AttentionFunction.apply(q.to(DEV), k.to(DEV), v.to(DEV), B, Lq, Lk, E, nhead, 0.0, seed), plain)
    assert not torch.equal(out, plain)
    other = ops.AttentionFunction.apply(q.to(DEV), k.to(DEV), v.to(DEV), B, Lq, Lk, E, nhead, p, seed + 1)
    assert not torch.equal(other, out)                                            # another seed: another mask


def test_mha_applies_the_dropout_to_1296_keys():
    """fusion_train._mha with p = 0.1 on the small head's cross-attention shape (20 queries x 1296 keys): the seed is the
    first draw after torch.manual_seed; output and the gradients towards every parameter and both inputs against the float64
    composition with that seed's mask.  (Before the key limit fell, _mha ran this shape without the dropout.)"""
    from isfusion_amd import fusion_ops as ops, fusion_train as tr
    B, Lq, Lk, E, nhead, p, s = 2, 20, 1296, 128, 8, 0.1, 77
    attn = torch.nn.MultiheadAttention(E, nhead)
    with torch.no_grad():
        for i, t in enumerate(attn.parameters()):
            t.copy_(rnd(t.shape, 500 + i, 0.5 if t.dim() == 1 else E ** -0.5))
    xq, kv, w = rnd((B * Lq, E), 91), rnd((B * Lk, E), 92), rnd((B * Lq, E), 93)
    torch.manual_seed(s)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    attn = attn.to(DEV)
    xg, kg = xq.to(DEV).requires_grad_(), kv.to(DEV).requires_grad_()
    torch.manual_seed(s)
    out = tr._mha(xg, kg, kg, attn, B, Lq, Lk, nhead, p)
    (out * w.to(DEV)).sum().backward()
    prm = {n: t.detach().cpu().double().requires_grad_() for n, t in attn.named_parameters()}
    xr, kr = xq.double().requires_grad_(), kv.double().requires_grad_()
    mask = ops.attention_keep_mask(seed, B, nhead, Lq, Lk, p)
    ref = H.f64_mha(prm["in_proj_weight"], prm["in_proj_bias"], prm["out_proj.weight"], prm["out_proj.bias"], xr, kr, kr,
                    B, Lq, Lk, nhead, mask, p)
    (ref * w.double()).sum().backward()
    assert rel_err(out, ref) < 1e-5
    assert rel_err(xg.grad, xr.grad) < 1e-4 and rel_err(kg.grad, kr.grad) < 1e-4
    for n, t in attn.named_parameters():
        assert rel_err(t.grad, prm[n].grad) < 1e-4, n
    # and it IS the dropout: without the mask the reference is elsewhere
    plain = H.f64_mha(prm["in_proj_weight"], prm["in_proj_bias"], prm["out_proj.weight"], prm["out_proj.bias"], xr, kr, kr,
                      B, Lq, Lk, nhead)
    assert rel_err(out, plain) > 1e-3


# ------------------------------------------------------------------------------------------------------------ the head
KEYS = ("center", "height", "dim", "rot", "vel", "heatmap", "dense_heatmap")


def _small_head(dropout, switch):
    from fusion_common import HEAD_CONFIGS, HEAD_SEED, head_input, head_kwargs
    from isfusion_amd.fusion_modules import seeded_state_dict
    from isfusion_amd.transfusion_head import TransFusionHeadV2
    cfg = HEAD_CONFIGS["small"]
    head = TransFusionHeadV2(dropout=dropout, **head_kwargs(cfg))
    head.load_state_dict(seeded_state_dict(head, HEAD_SEED))
    head.cross_attention_dropout = switch
    return head.to(DEV), head_input(cfg).to(DEV)


def test_head_with_cross_attention_dropout_matches_the_float64_head(monkeypatch):
    """the small head (B = 2, 1296 keys, 20 proposals), dropout 0.1, training mode, the switch on, F.dropout the identity: the
    two hash-seeded attention masks are the only stochastic ops left, their seeds the first two draws after
    torch.manual_seed (self-attention, then cross-attention).  Every output, the input gradient and every parameter
    gradient against the float64 head with both masks: measure and bounds of
    test_head_forward_train_gradients_match_float64_torch (1e-4 outputs, 2e-4 gradients)."""
    from isfusion_amd import fusion_ops as ops
    p, s = 0.1, 11
    head, x = _small_head(p, True)
    head.train()
    monkeypatch.setattr(torch.nn.functional, "dropout", lambda t, *a, **k: t)
    torch.manual_seed(s)
    seed_self, seed_cross = (int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(2))
    xg = x.clone().requires_grad_(True)
    torch.manual_seed(s)
    out = head.forward_train(xg)[0][0]
    B, _, X, _ = x.shape
    P, nhead = head.num_proposals, head.decoder[0].nhead
    self_mask = ops.attention_keep_mask(seed_self, B, nhead, P, P, p)
    cross_mask = ops.attention_keep_mask(seed_cross, B, nhead, P, X * X, p)
    ref, prm, xd = H.f64_head(head, x, head.last_top_index, head.query_labels, B, X, P, self_mask, cross_mask, p, nhead)
    g = torch.Generator().manual_seed(3)
    wts = {k: torch.randn(ref[k].shape, generator=g, dtype=torch.float64) for k in KEYS}
    for k in KEYS:
        assert rel_err(out[k], ref[k]) < 1e-4, k
    sum((out[k] * wts[k].float().to(DEV)).sum() for k in KEYS).backward()
    sum((ref[k] * wts[k]).sum() for k in KEYS).backward()
    assert rel_err(xg.grad, xd.grad) < 2e-4
    missing = [n for n, t in head.named_parameters() if t.grad is None]
    assert not missing, missing
    for n, t in head.named_parameters():
        assert rel_err(t.grad, prm[n].grad) < 2e-4, n
    # the cross mask matters: the same float64 head without it is elsewhere
    other = H.f64_head(head, x, head.last_top_index, head.query_labels, B, X, P, self_mask, None, p, nhead)[0]
    assert max(rel_err(out[k], other[k]) for k in KEYS if k != "dense_heatmap") > 1e-3


def _train_run(head, x, seed):
    head.zero_grad()
    torch.manual_seed(seed)
    out = head.forward_train(x)[0][0]
    sum(out[k].square().sum() for k in KEYS).backward()
    return {k: out[k].detach().clone() for k in KEYS}, {n: t.grad.clone() for n, t in head.named_parameters()}


def test_head_switch_behaviour():
    """off: the warning about the missing op, naming the switch; on: other outputs under the same torch seed, bit-identical
    under isfusion_amd.deterministic(); eval(): the switch changes nothing"""
    import isfusion_amd
    from isfusion_amd.transfusion_head import TransFusionHeadV2
    head, x = _small_head(0.1, False)
    head.train()
    TransFusionHeadV2._warned_cross_dropout = False
    with pytest.warns(UserWarning, match="cross_attention_dropout"):
        off, _ = _train_run(head, x, 5)
    head.cross_attention_dropout = True
    TransFusionHeadV2._warned_cross_dropout = False
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                   # switched on: nothing to warn about
        on, _ = _train_run(head, x, 5)
    assert not TransFusionHeadV2._warned_cross_dropout
    assert any(not torch.equal(on[k], off[k]) for k in KEYS if k != "dense_heatmap")
    with isfusion_amd.deterministic():
        a, ga = _train_run(head, x, 5)
        b, gb = _train_run(head, x, 5)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    # eval(): no dropout anywhere, the switch is not looked at.  (Gradients stay enabled, so forward_train runs on its HIP
    # Functions, and deterministic mode, because two plain calls of it differ in the last bit of the heat-map convs.)
    head.eval()
    outs = []
    for switch in (True, False):
        head.cross_attention_dropout = switch
        with isfusion_amd.deterministic():
            outs.append(head.forward_train(x)[0][0])
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
