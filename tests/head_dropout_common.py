"""float64 stock-torch compositions for tests/test_gpu_attention_dropout_keys.py: nn.MultiheadAttention's arithmetic and
the detection head's training-mode forward (forward_single, transfusion_head_v2.py:771-892, batch statistics) with the
dropout on the attention PROBABILITIES given as explicit keep masks (fusion_ops.attention_keep_mask of the seeds the
kernels drew), every other dropout the identity.  A restatement of its own: it shares no code with the head under test."""
import torch

F = torch.nn.functional


def masked_attention(q, k, v, B, Lq, Lk, nhead, mask=None, p=0.0):
    """softmax(q k^T / sqrt(hd)) [* mask / (1 - p)] v on row-major [B*L, E] float64 tokens; mask [B, nhead, Lq, Lk] bool"""
    E = q.shape[1]
    hd = E // nhead
    sp = lambda t, L: t.view(B, L, nhead, hd).transpose(1, 2)
    prob = torch.softmax(sp(q, Lq) @ sp(k, Lk).transpose(-1, -2) / hd ** 0.5, -1)
    if mask is not None:
        prob = prob * mask.to(prob.dtype) / (1.0 - p)
    return (prob @ sp(v, Lk)).transpose(1, 2).reshape(B * Lq, E)


def f64_mha(w_in, b_in, w_out, b_out, q_in, k_in, v_in, B, Lq, Lk, nhead, mask=None, p=0.0):
    """nn.MultiheadAttention on row-major tokens from its four parameter tensors (float64)"""
    E = q_in.shape[1]
    q = q_in @ w_in[:E].t() + b_in[:E]
    k = k_in @ w_in[E:2 * E].t() + b_in[E:2 * E]
    v = v_in @ w_in[2 * E:].t() + b_in[2 * E:]
    return masked_attention(q, k, v, B, Lq, Lk, nhead, mask, p) @ w_out.t() + b_out


def f64_head(head, x, cell, labels, B, X, P, self_mask=None, cross_mask=None, p=0.0, nhead=8, num_classes=10):
    """the head's training-mode forward on the given proposals (cell, labels as the head under test mined them), float64 on
    the CPU, batch statistics in every BatchNorm -> (outputs, {name: parameter leaf}, input leaf)"""
    prm = {n: t.detach().cpu().double().requires_grad_(True) for n, t in head.named_parameters()}
    xd = x.detach().cpu().double().requires_grad_(True)
    bn = lambda t, n: F.batch_norm(t, None, None, prm[n + ".weight"], prm[n + ".bias"], True, 0.0, 1e-5)
    lin = lambda t, n: t @ prm[n + ".weight"].t() + prm[n + ".bias"]
    conv1 = lambda t, n: t @ prm[n + ".weight"][:, :, 0].t() + (prm[n + ".bias"] if n + ".bias" in prm else 0.0)
    feat = F.conv2d(xd, prm["shared_conv.weight"], prm["shared_conv.bias"], padding=1)
    h = F.relu(bn(F.conv2d(feat, prm["heatmap_head.0.conv.weight"], None, padding=1), "heatmap_head.0.bn"))
    dense = F.conv2d(h, prm["heatmap_head.1.weight"], prm["heatmap_head.1.bias"], padding=1)
    E, HW = feat.shape[1], X * X
    rows = feat.flatten(2).transpose(1, 2)                                               # [B, HW, E]
    cell, labels = cell.cpu(), labels.cpu()
    query = rows.gather(1, cell[:, :, None].expand(-1, -1, E))
    query = (query + conv1(F.one_hot(labels, num_classes).double(), "class_encoding")).reshape(B * P, E)
    centres = torch.arange(X, dtype=torch.float64) + 0.5
    bev = torch.stack(torch.meshgrid(centres, centres, indexing="ij"), 0).view(2, -1).t()  # [HW, 2]
    qpos = bev[cell]                                                                     # [B, P, 2]

    def pos_embed(n, xy):
        t = F.relu(bn(conv1(xy.reshape(-1, 2), n + ".position_embedding_head.0"), n + ".position_embedding_head.1"))
        return conv1(t, n + ".position_embedding_head.3")

    def mha(n, qi, kvi, Lq, Lk, mask):
        return f64_mha(prm[n + ".in_proj_weight"], prm[n + ".in_proj_bias"], prm[n + ".out_proj.weight"],
                       prm[n + ".out_proj.bias"], qi, kvi, kvi, B, Lq, Lk, nhead, mask, p)

    ln = lambda t, n: F.layer_norm(t, (E,), prm[n + ".weight"], prm[n + ".bias"], 1e-5)
    d = "decoder.0"
    qpe = pos_embed(d + ".self_posembed", qpos)
    kv = (rows + pos_embed(d + ".cross_posembed", bev)[None]).reshape(B * HW, E)
    xq = query + qpe
    query = ln(query + mha(d + ".self_attn", xq, xq, P, P, self_mask), d + ".norm1")
    query = ln(query + mha(d + ".multihead_attn", query + qpe, kv, P, HW, cross_mask), d + ".norm2")
    query = ln(query + lin(F.relu(lin(query, d + ".linear1")), d + ".linear2"), d + ".norm3")
    res = {}
    for name in head.prediction_heads[0].heads:
        n = f"prediction_heads.0.{name}"
        t = F.relu(bn(conv1(query, n + ".0.conv"), n + ".0.bn"))
        res[name] = conv1(t, n + ".1").view(B, P, -1).permute(0, 2, 1)
    res["center"] = res["center"] + qpos.permute(0, 2, 1)
    res["dense_heatmap"] = dense
    return res, prm, xd
