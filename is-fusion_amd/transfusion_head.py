"""TransFusionHeadV2.forward_single (mmdet3d/models/dense_heads/transfusion_head_v2.py:771-892):
BEV feature map [B, 512, 180, 180] -> shared conv -> heat-map -> sigmoid + 3x3 NMS + top-200 proposals (the same fused
kernel as the encoder's instance mining) -> one transformer decoder layer (200-query self-attention, 200 x 32400
cross-attention over the BEV map with learned position embeddings, FFN) -> per-proposal regression / class heads.

Parameter / sub-module names equal the reference's (96 state-dict keys; checked with ``load_state_dict(strict=True)``
into the reference class in tests/golden/make_golden_head.py).  Inference: ``forward`` / ``forward_split`` and the box
decoding ``get_bboxes`` (isf_decode_boxes, below) are built and pinned by reference goldens.  Training:
``forward_train`` (the same forward with gradients on the training autograd Functions), ``get_targets`` and ``loss``
(head_loss.py / isf_head_loss.hip, pinned by tests/golden/head_loss_ref.npz).

HIP path: the two 3x3 convs on the f16x3 sparse-conv kernel over the dense grid, top-k through ``isf_instance_topk``,
all Linear layers through ``isf_linear_forward`` (the key / value projection of the 32400 x B BEV tokens folds the
learned key position embedding into a per-cell table), attention through ``isf_attention_forward`` (keys split into
512-key chunks + merge).  The 2 -> 128 position MLPs, the 128 -> 10 heat-map conv and the Conv1d prediction heads on 200
proposals stay stock torch ops (tiny, channel counts below the MFMA tile).
"""
import copy
import warnings

import torch
from torch import nn

from . import fusion_ops as ops
from . import head_loss
from ._lib import require_cuda as _lib_require_cuda
from .dense_conv import PackedConvBN, SplitMap
from .fusion_modules import PositionEmbeddingLearned, _SelfAttn
from .spconv import F16X3_CHANNELS, from_split


class _ConvModule1d(nn.Sequential):
    """mmcv ConvModule(conv_cfg=Conv1d, norm_cfg=BN1d, bias='auto'): conv (no bias) / bn / activate"""

    def __init__(self, cin, cout):
        super().__init__()
        self.add_module("conv", nn.Conv1d(cin, cout, 1, bias=False))
        self.add_module("bn", nn.BatchNorm1d(cout))
        self.add_module("activate", nn.ReLU(inplace=True))


class _ConvModule2d(nn.Sequential):
    def __init__(self, cin, cout):
        super().__init__()
        self.add_module("conv", nn.Conv2d(cin, cout, 3, padding=1, bias=False))
        self.add_module("bn", nn.BatchNorm2d(cout))
        self.add_module("activate", nn.ReLU(inplace=True))


class FFN(nn.Module):
    """transfusion_head_v2.py:505-590: one Conv1d stack per output (`center`, `height`, ...)"""

    def __init__(self, in_channels, heads, head_conv=64):
        super().__init__()
        self.heads = heads
        for head, (classes, num_conv) in heads.items():
            layers, c = [], in_channels
            for _ in range(num_conv - 1):
                layers.append(_ConvModule1d(c, head_conv))
                c = head_conv
            layers.append(nn.Conv1d(c, classes, 1))
            setattr(self, head, nn.Sequential(*layers))

    def forward(self, x):
        return {head: getattr(self, head)(x) for head in self.heads}


class TransformerDecoderLayer(nn.Module):
    """transfusion_head_v2.py:42-120 parameter layout"""

    def __init__(self, d_model, nhead, dim_feedforward):
        super().__init__()
        self.nhead = nhead
        self.self_attn = _SelfAttn(d_model)
        self.multihead_attn = _SelfAttn(d_model)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.norm3 = nn.LayerNorm(d_model)
        self.self_posembed = PositionEmbeddingLearned(2, d_model)
        self.cross_posembed = PositionEmbeddingLearned(2, d_model)


class TransFusionHeadV2(nn.Module):
    _warned_cross_dropout = False
    cross_attention_dropout = False   # a plain attribute: not a parameter, buffer or constructor argument.  True: in training
                                      # mode with dropout > 0, forward_train applies the decoder layer's dropout to the
                                      # probabilities of the proposals x BEV-cells cross-attention (see forward_train)

    def __init__(self, num_proposals=200, auxiliary=True, in_channels=512, hidden_channel=128, num_classes=10,
                 num_decoder_layers=1, num_heads=8, nms_kernel_size=3, ffn_channel=256, common_heads=None,
                 num_heatmap_convs=2, test_cfg=None, bbox_coder=None, dense_conv="hip", train_cfg=None, loss_cls=None,
                 loss_bbox=None, loss_heatmap=None, dropout=0.1, **kwargs):
        super().__init__()
        self.num_classes, self.num_proposals, self.auxiliary = num_classes, num_proposals, auxiliary
        self.dropout = float(dropout)     # TransformerDecoderLayer dropouts (transfusion_head_v2.py:42-60), forward_train only
        # training: the reference's names (transfusion_head_v2.py:642-646, 758-766); None = the shipped configuration
        self.train_cfg = dict(train_cfg) if train_cfg is not None else None
        self.loss_cls = dict(loss_cls or head_loss.SHIPPED_LOSS_CLS)
        self.loss_bbox = dict(loss_bbox or head_loss.SHIPPED_LOSS_BBOX)
        self.loss_heatmap = dict(loss_heatmap or head_loss.SHIPPED_LOSS_HEATMAP)
        head_loss.check_loss_cfgs(self.loss_cls, self.loss_bbox, self.loss_heatmap)
        if self.train_cfg is not None:
            head_loss.check_train_cfg(self.train_cfg)
        self.num_heads, self.num_decoder_layers, self.nms_kernel_size = num_heads, num_decoder_layers, nms_kernel_size
        self.test_cfg = test_cfg or dict(dataset="nuScenes", grid_size=[1440, 1440, 40], out_size_factor=8)
        self.dense_conv = dense_conv
        # TransFusionBBoxCoder arguments (configs/isfusion/isfusion_0075voxel.py:130-138); decoding runs in one kernel
        self.bbox_coder = dict(pc_range=[-54.0, -54.0], voxel_size=[0.075, 0.075], out_size_factor=8,
                               post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], score_threshold=0.0,
                               code_size=10)
        self.bbox_coder.update({k: v for k, v in (bbox_coder or {}).items() if k != "type"})
        common_heads = common_heads or dict(center=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2))
        self.shared_conv = nn.Conv2d(in_channels, hidden_channel, 3, padding=1, bias=True)
        self.heatmap_head = nn.Sequential(_ConvModule2d(hidden_channel, hidden_channel),
                                          nn.Conv2d(hidden_channel, num_classes, 3, padding=1, bias=True))
        self.class_encoding = nn.Conv1d(num_classes, hidden_channel, 1)
        self.decoder = nn.ModuleList([TransformerDecoderLayer(hidden_channel, num_heads, ffn_channel)
                                      for _ in range(num_decoder_layers)])
        self.prediction_heads = nn.ModuleList()
        for _ in range(num_decoder_layers):
            heads = copy.deepcopy(common_heads)
            heads.update(dict(heatmap=(num_classes, num_heatmap_convs)))
            self.prediction_heads.append(FFN(hidden_channel, heads))
        self.x_size = self.test_cfg["grid_size"][0] // self.test_cfg["out_size_factor"]
        self.y_size = self.test_cfg["grid_size"][1] // self.test_cfg["out_size_factor"]

    # ------------------------------------------------------------------------------------------------ pieces
    def _bev_pos(self, device):
        """create_2D_grid (:728-738): [1, X*Y, 2] cell centres, cell n = i*Y + j -> (i + .5, j + .5)"""
        gx = torch.linspace(0, self.x_size - 1, self.x_size, device=device) + 0.5
        gy = torch.linspace(0, self.y_size - 1, self.y_size, device=device) + 0.5
        bx, by = torch.meshgrid(gx, gy, indexing="ij")
        return torch.stack([bx, by], 0).view(1, 2, -1).permute(0, 2, 1)

    def _packed(self, device):
        c = ops._cache(self, device)                    # dropped when any parameter / buffer of the head changes
        if "shared" not in c:
            c["shared"] = PackedConvBN(self.shared_conv, None, relu=False)
            c["hm0"] = PackedConvBN(self.heatmap_head[0].conv, self.heatmap_head[0].bn, relu=True)
            c["hm1"] = PackedConvBN(self.heatmap_head[1], None, relu=False)   # 128 -> 10 (columns zero-padded to 32)
            bev_pos = self._bev_pos(device)
            c["bev_pos"] = bev_pos
            c["bev_pos_tok"] = bev_pos[0].contiguous()                            # [HW, 2] for isf_head_query_init
            c["layers"] = []
            E = self.shared_conv.out_channels
            for l in self.decoder:
                sa, ca = l.self_attn, l.multihead_attn
                ws, bs = sa.in_proj_weight.detach().float(), sa.in_proj_bias.detach().float()
                wc, bc = ca.in_proj_weight.detach().float(), ca.in_proj_bias.detach().float()
                # key = value = feat + key_pos_embed (:104-106): (feat + pos) W + b = feat W + (pos W + b), the second
                # term is input independent -> per-cell table added in the GEMM epilogue
                kpe = ops._pos_embed(l.cross_posembed, bev_pos)[0]                    # [HW, E]
                # the proposals sit on cell centres (query_pos = bev_pos[top_index]): their self-attention position
                # embedding is a row of this per-cell table (same MLP, same inputs) -- no GEMMs per forward
                qtab = ops._pos_embed(l.self_posembed, bev_pos)[0].contiguous()
                table = (kpe.double() @ wc[E:].double().t()).float().contiguous()     # [HW, 2E]
                c["layers"].append(dict(
                    s_qkv=ops.PackedLinear(ws, bs), s_out=ops.PackedLinear(sa.out_proj.weight, sa.out_proj.bias),
                    c_q=ops.PackedLinear(wc[:E], bc[:E]), c_kv=ops.PackedLinear(wc[E:], bc[E:]), kv_table=table,
                    c_out=ops.PackedLinear(ca.out_proj.weight, ca.out_proj.bias),
                    l1=ops.PackedLinear(l.linear1.weight, l.linear1.bias),
                    l2=ops.PackedLinear(l.linear2.weight, l.linear2.bias), qpe_table=qtab))
            c["pred"] = [self._pack_prediction_heads(ffn) for ffn in self.prediction_heads]
        return c

    @staticmethod
    def _pack_prediction_heads(ffn):
        """The per-output Conv1d stacks of an FFN (transfusion_head_v2.py:505-590; kernel size 1 = per-proposal linear
        layers) as GEMM pairs: the first layers of a GROUP of outputs side by side (eval BatchNorm folded, ReLU in the
        epilogue), their last layers as one block-diagonal matrix.  Groups of 4 / 2 / 1 outputs keep the hidden width
        (64 each) inside what the linear kernel tiles (<= 256): the shipped six outputs are 4 + 2 = four launches for 12
        convolutions + 6 BatchNorms + 6 ReLUs.  -> None when a stack is not the shipped (conv-bn-relu, conv) shape or
        width; the caller then runs the modules."""
        heads = []
        for name in ffn.heads:
            seq = getattr(ffn, name)
            if len(seq) != 2 or not isinstance(seq[0], _ConvModule1d) or not isinstance(seq[1], nn.Conv1d):
                return None
            conv, bn, last = seq[0].conv, seq[0].bn, seq[1]
            if conv.weight.shape[0] != 64 or conv.weight.shape[1] not in F16X3_CHANNELS:
                return None
            scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach().float()
            heads.append((name, conv.weight.detach().float()[:, :, 0] * scale[:, None],
                          (bn.bias - bn.running_mean * scale).detach().float(), last.weight.detach().float()[:, :, 0],
                          last.bias.detach().float()))
        groups, i = [], 0
        while i < len(heads):
            n = 4 if len(heads) - i >= 4 else 2 if len(heads) - i >= 2 else 1
            grp = heads[i:i + n]
            i += n
            hid = 64 * n
            n_out = sum(h[3].shape[0] for h in grp)
            w2 = grp[0][1].new_zeros(((n_out + 15) // 16 * 16, hid))      # the linear kernel writes 16-column tiles
            b2 = grp[0][1].new_zeros((w2.shape[0],))
            cols, r = [], 0
            for k, (name, _, _, w, b) in enumerate(grp):
                w2[r:r + w.shape[0], 64 * k:64 * (k + 1)] = w
                b2[r:r + w.shape[0]] = b
                cols.append((name, r, r + w.shape[0]))
                r += w.shape[0]
            groups.append(dict(l1=ops.PackedLinear(torch.cat([h[1] for h in grp], 0), torch.cat([h[2] for h in grp], 0)),
                               l2=ops.PackedLinear(w2, b2), cols=cols))
        return groups

    @torch.no_grad()
    def forward_split(self, maps):
        """engine-level entry (ISFusionPtsPath.forward_pts): `maps` = SECONDFPN.forward_split(...) -- the neck output as
        split-format token matrices of the UN-permuted BEV map M [B, C, H, W] (the reference hands over
        P = M.permute(0, 1, 3, 2)).  Same result as forward_single(P): the 3x3 convolutions run with transposed taps on
        M's tokens and only the 10-channel heat-map is permuted."""
        assert self.dense_conv == "hip", "forward_split is the HIP path"
        return [self.forward_single(None, maps_yx=maps)[0]]

    @torch.no_grad()
    def forward_single(self, inputs, img_inputs=None, metas=None, maps_yx=None):
        """inputs [B, in_channels, X, Y] -> [dict(center, height, dim, rot, vel, heatmap, query_heatmap_score,
        dense_heatmap)] (one dict: num_decoder_layers results concatenated along the proposal axis when auxiliary)"""
        assert not self.training, "isfusion_amd.TransFusionHeadV2 is the inference path (eval mode)"
        E = self.shared_conv.out_channels
        tok_of_cell = None      # BEV cell x*Y + y (the head's indexing) -> row of feat_tok; None = identity
        if maps_yx is not None:
            m0 = maps_yx[0]
            B, X, Y = m0.B, m0.W, m0.H                                             # the head's X is M's W axis
            HW = X * Y
            dev = m0.data.device
            c = self._packed(dev)
            feat = c["shared"](maps_yx, transpose=True)                            # SplitMap of M: token (b, y, x)
            hm_mid = c["hm0"](feat, transpose=True)                                # SplitMap [B, E, H, W]
            feat_tok = from_split(feat.data, (B * HW, E))
            dense_heatmap = c["hm1"](hm_mid, transpose=True).to_nchw(self.heatmap_head[1].out_channels)
            dense_heatmap = dense_heatmap.permute(0, 1, 3, 2).contiguous()         # [B, classes, X, Y]
            key = ("tok_of_cell", X, Y)
            if key not in c:
                cell = torch.arange(HW, device=dev)
                c[key] = (cell % Y) * X + torch.div(cell, Y, rounding_mode="floor")           # (x, y) -> y*W + x
                c[("cell_of_tok", X, Y)] = ((cell % X) * Y + torch.div(cell, X, rounding_mode="floor")).int()
            tok_of_cell = c[key]
        else:
            B, _, X, Y = inputs.shape
            HW = X * Y
            dev = inputs.device
            c = self._packed(dev)
            if self.dense_conv == "hip":
                maps = [SplitMap.from_nchw(inputs, off, min(256, inputs.size(1) - off))
                        for off in range(0, inputs.size(1), 256)]
                feat = c["shared"](maps)                                          # SplitMap [B, E, X, Y]
                dense_heatmap = c["hm1"](c["hm0"](feat)).to_nchw(self.heatmap_head[1].out_channels).contiguous()
                feat_tok = from_split(feat.data, (B * HW, E))                     # token-major fp32
            else:
                lidar_feat = self.shared_conv(inputs)
                dense_heatmap = self.heatmap_head[1](self.heatmap_head[0](lidar_feat))
                feat_tok = ops.to_tokens(lidar_feat)
        pool1 = (8, 9) if self.test_cfg["dataset"] == "nuScenes" else (1, 2)
        top32, raw32, masked = ops.instance_topk(dense_heatmap, self.num_proposals, self.nms_kernel_size, pool1,
                                                 return_masked=True, as_int32=True)
        # labels, positions, query = feature column + class_encoding(one_hot) (= column `class` of the 1x1 conv + bias),
        # the first layer's position embedding (the proposals sit on cell centres: a row of the per-cell table), query +
        # position and the proposals' heat-map scores: one launch (isf_head_query_init)
        ce = self.class_encoding
        ctab = c.get("class_table")
        if ctab is None:
            ctab = c["class_table"] = (ce.weight[:, :, 0].t() + ce.bias).detach().float().contiguous()
        query, qpe0, x0, query_pos, top_index, top_class, q_score = ops.head_query_init(
            top32, raw32, feat_tok, tok_of_cell, ctab, c["layers"][0]["qpe_table"], c["bev_pos_tok"], masked,
            self.num_classes)
        self.query_labels = top_class
        self.last_top_index = top_index   # BEV cell of every proposal (for inspection)
        P = self.num_proposals
        ret_dicts = []
        for i, (l, p) in enumerate(zip(self.decoder, c["layers"])):
            if i == 0:   # = self_posembed(query_pos): the proposals sit on cell centres; later layers use refined centres
                qpe, x = qpe0, x0
            else:
                qpe = ops._pos_embed(l.self_posembed, query_pos).reshape(B * P, E)
                x = query + qpe
            # self attention: q = k = v = query + pos (:98-101)
            qkv = ops.linear(x, p["s_qkv"])
            att = ops.attention(qkv, qkv[:, E:], qkv[:, 2 * E:], B, P, P, E, l.nhead, ldkv=3 * E)
            query = ops.linear(att, p["s_out"], residual=query, ln=l.norm1)
            # cross attention over the BEV map (:104-108)
            qc = ops.linear(query + qpe, p["c_q"])
            if tok_of_cell is None:
                idx = c.setdefault(("kv_index", B, HW), torch.arange(HW, device=dev, dtype=torch.int32).repeat(B))
            else:   # key token (b, y, x) takes the position row of its cell x*Y + y
                idx = c.setdefault(("kv_index_yx", B, X, Y), c[("cell_of_tok", X, Y)].repeat(B))
            kv = ops.linear(feat_tok, p["c_kv"], table=p["kv_table"], index=idx)                     # [B*HW, 2E]
            att = ops.attention(qc, kv, kv[:, E:], B, P, HW, E, l.nhead, ldkv=2 * E)
            query = ops.linear(att, p["c_out"], residual=query, ln=l.norm2)
            h = ops.linear(query, p["l1"], act=ops.ACT_RELU)
            query = ops.linear(h, p["l2"], residual=query, ln=l.norm3)
            pp = c["pred"][i] if self.dense_conv == "hip" else None
            if pp is not None:
                blocks = []
                for grp in pp:
                    o = ops.linear(ops.linear(query, grp["l1"], act=ops.ACT_RELU), grp["l2"])       # [B*P, columns]
                    blocks += [(n, o, a, b - a) for n, a, b in grp["cols"]]
                # every output as [B, c, P], center += query_pos, the next layer's positions: one launch
                res, query_pos = ops.head_scatter_predictions(blocks, B, P, query_pos.contiguous())
                res = {n: res[n] for n in self.prediction_heads[i].heads}      # the reference's key order
            else:
                res = self.prediction_heads[i](query.view(B, P, E).transpose(1, 2).contiguous())       # [B, E, P]
                res["center"] = res["center"] + query_pos.permute(0, 2, 1)
                query_pos = res["center"].detach().clone().permute(0, 2, 1)
            ret_dicts.append(res)
        ret_dicts[0]["query_heatmap_score"] = q_score
        ret_dicts[0]["dense_heatmap"] = dense_heatmap
        if not self.auxiliary:
            return [ret_dicts[-1]]
        new_res = {}
        for key in ret_dicts[0].keys():
            if key not in ("dense_heatmap", "dense_heatmap_old", "query_heatmap_score"):
                # (one decoder layer, the shipped head: the tensor itself -- torch.cat of one tensor is a copy launch)
                new_res[key] = torch.cat([r[key] for r in ret_dicts], dim=-1) if len(ret_dicts) > 1 else ret_dicts[0][key]
            else:
                new_res[key] = ret_dicts[0][key]
        return [new_res]

    def forward(self, feats, img_feats=None, metas=None):
        """:894-908: one level"""
        if isinstance(feats, torch.Tensor):
            feats = [feats]
        # multi_apply transposes the per-level lists: a 1-tuple holding the list of per-level result dicts
        return ([self.forward_single(f, None, metas)[0] for f in feats],)

    def forward_train(self, feats):
        """forward_single (:771-892) in training mode WITH gradients, on the training autograd Functions: the 3x3 convs
        through dense_train.conv_stack, top-k proposals through isf_instance_topk (no gradient), differentiable gathers
        of the proposal features, the decoder layer's attention through fusion_train._mha (HIP linear + attention
        kernels), FFN / layer norms, the prediction heads as HIP linears + bn1d_relu.  Dropout p = self.dropout where the
        reference applies it (dropout1..3 and the FFN dropout; the attention-probability dropout of the 200 x 200
        self-attention on the dropout kernels).  The 200 x 32400 cross-attention gets its probability dropout
        (MultiheadAttention(dropout=0.1), transfusion_head_v2.py:49, :490) when `cross_attention_dropout` is True: the same
        hash-seeded kernels, the backward by key splits (isf_attention_bwd.hip).  The switch is off by default, and then a
        warning says once that the op is missing: tests/test_gpu_head_train.py records a 30-step loss curve with dropout
        on, and the extra mask moves that curve and, through its seed, every later random draw of the step -- turning it
        on by default is a change of its own with a re-recorded curve.  feats: [B, in_channels, X, Y] or a one-element
        list -> ([dict],) as forward returns it."""
        from . import dense_train, fusion_train
        x = feats[0] if isinstance(feats, (list, tuple)) else feats
        _lib_require_cuda(x)
        B, _, X, Y = x.shape
        HW, P, C = X * Y, self.num_proposals, self.num_classes
        E = self.shared_conv.out_channels
        p, tr = self.dropout, self.training
        feat = dense_train.conv_stack(self.shared_conv, x)                                # NCHW view of [B*HW, E] rows
        # (128 -> 10 classes: the kernels on 32 zero-padded columns, the bias added behind them)
        dense_heatmap = dense_train.conv_stack(self.heatmap_head[1], dense_train.conv_stack(self.heatmap_head[0], feat),
                                               narrow=not fusion_train.STOCK_CONVS)
        dense_heatmap = dense_heatmap.float().contiguous()
        pool1 = (8, 9) if self.test_cfg["dataset"] == "nuScenes" else (1, 2)
        top, raw, masked = ops.instance_topk(dense_heatmap.detach(), P, self.nms_kernel_size, pool1, return_masked=True)
        cell, labels = top, torch.div(raw, HW, rounding_mode="floor")
        self.query_labels = labels
        self.last_top_index = cell
        rows = dense_train.to_rows(feat)                                                   # [B*HW, E], row b*HW + cell
        query = ops.gather_cells(rows.view(B, HW, E), cell, channels_last=True)             # [B, P, E]
        one_hot = torch.nn.functional.one_hot(labels, C).float()                          # class_encoding (Conv1d, k=1)
        query = (query + torch.nn.functional.linear(one_hot, self.class_encoding.weight[:, :, 0],
                                                    self.class_encoding.bias)).reshape(B * P, E)
        bev_pos = self._bev_pos(x.device)                                                  # [1, HW, 2]
        query_pos = bev_pos[0][cell]                                                       # [B, P, 2]
        drop = torch.nn.functional.dropout
        ln = torch.nn.functional.layer_norm
        cross_p = p if tr and self.cross_attention_dropout else 0.0
        if p > 0.0 and tr and not self.cross_attention_dropout and not TransFusionHeadV2._warned_cross_dropout:
            TransFusionHeadV2._warned_cross_dropout = True
            warnings.warn("TransFusionHeadV2.forward_train: no dropout on the attention probabilities of the 200 x 32400 "
                          "cross-attention (set cross_attention_dropout = True to apply it); the output dropout is applied")
        ret_dicts = []
        for i, l in enumerate(self.decoder):
            qpe = ops._pos_embed(l.self_posembed, query_pos).reshape(B * P, E)
            kpe = ops._pos_embed(l.cross_posembed, bev_pos)[0]                             # [HW, E], the same per sample
            xq = query + qpe                                                               # q = k = v (:98-101)
            sa = fusion_train._mha(xq, xq, xq, l.self_attn, B, P, P, l.nhead, p if tr else 0.0)
            query = ln(query + drop(sa, p, tr), (E,), l.norm1.weight, l.norm1.bias, l.norm1.eps)
            kv = (rows.view(B, HW, E) + kpe[None]).reshape(B * HW, E)                      # key = value = feat + pos
            ca = fusion_train._mha(query + qpe, kv, kv, l.multihead_attn, B, P, HW, l.nhead, cross_p)
            query = ln(query + drop(ca, p, tr), (E,), l.norm2.weight, l.norm2.bias, l.norm2.eps)
            h = drop(torch.relu(fusion_train.linear(query, l.linear1)), p, tr)
            query = ln(query + drop(fusion_train.linear(h, l.linear2), p, tr), (E,), l.norm3.weight, l.norm3.bias,
                       l.norm3.eps)
            res = {}
            for name in self.prediction_heads[i].heads:
                res[name] = self._train_pred_head(getattr(self.prediction_heads[i], name), query, B, P)
            res["center"] = res["center"] + query_pos.permute(0, 2, 1)
            query_pos = res["center"].detach().permute(0, 2, 1)
            ret_dicts.append(res)
        ret_dicts[0]["query_heatmap_score"] = masked.view(B, C, HW).gather(2, cell[:, None, :].expand(-1, C, -1))
        ret_dicts[0]["dense_heatmap"] = dense_heatmap
        if not self.auxiliary:
            return ([ret_dicts[-1]],)
        out = {}
        for key in ret_dicts[0]:
            if key in ("dense_heatmap", "query_heatmap_score"):
                out[key] = ret_dicts[0][key]
            else:
                out[key] = torch.cat([r[key] for r in ret_dicts], -1) if len(ret_dicts) > 1 else ret_dicts[0][key]
        return ([out],)

    @staticmethod
    def _train_pred_head(seq, query, B, P):
        """one FFN output (:505-590; Conv1d k=1 = per-proposal linear) on [B*P, E] rows -> [B, n, P]: the HIP linear
        (the last layer's rows zero-padded to 32, which both the forward's 16-column tiles and the backward's
        32-deep K take) and bn1d_relu for the ConvModule1d layers"""
        from .fusion_train import linear_w
        from .norm import bn1d_relu
        h = query
        for m in seq:
            if isinstance(m, _ConvModule1d):
                h = bn1d_relu(m.bn, linear_w(h, m.conv.weight[:, :, 0]), relu=True)
            else:
                n = m.weight.shape[0]
                pad = (-n) % 32            # 32: the backward's dX GEMM reads these rows as its K
                w = torch.nn.functional.pad(m.weight[:, :, 0], (0, 0, 0, pad))
                b = torch.nn.functional.pad(m.bias, (0, pad)) if m.bias is not None else None
                h = linear_w(h, w, b)[:, :n]
        return h.reshape(B, P, -1).permute(0, 2, 1)

    def get_targets(self, gt_bboxes_3d, gt_labels_3d, preds_dict):
        """:910-960 for the whole batch on the device (isf_head_loss.hip: heat-map targets, assignment cost, linear sum
        assignment, target assembly).  gt_bboxes_3d: per sample a [G, 9] tensor in the LiDARInstance3DBoxes layout
        (bottom centre) or an object with such a `.tensor`; preds_dict: the per-layer list of prediction dicts.
        -> (labels, label_weights, bbox_targets, bbox_weights, ious, num_pos, matched_ious, heatmap); num_pos and
        matched_ious are device scalars (no host sync)."""
        return head_loss.get_targets(self, gt_bboxes_3d, gt_labels_3d, preds_dict[0])

    def loss(self, gt_bboxes_3d, gt_labels_3d, preds_dicts, ins_heatmap=None, **kwargs):
        """:1143-1276 -> dict(loss_heatmap, loss_heatmap_ins (when ins_heatmap is given), layer_-1_loss_cls,
        layer_-1_loss_bbox, matched_ious); the losses are autograd Functions over the fused loss kernels."""
        return head_loss.loss(self, gt_bboxes_3d, gt_labels_3d, preds_dicts, ins_heatmap)

    # the per-dataset task table of get_bboxes (:1314-1340): (class indices, radius); radius <= 0 = no NMS
    NMS_TASKS = {
        "nuScenes": [([0, 1, 2, 3, 4, 5, 6, 7], -1.0), ([8], 0.175), ([9], 0.175)],
        "Waymo": [([0], 0.7), ([1], 0.7), ([2], 0.7)],
    }

    def _nms_plan(self):
        """test_cfg -> None (nms_type None) or the segmented-NMS arguments of the task table"""
        nms_type = self.test_cfg.get("nms_type")
        if nms_type is None:
            return None
        if nms_type not in ("circle", "rotate"):
            raise NotImplementedError(f"get_bboxes: nms_type={nms_type!r}; 'circle', 'rotate' or None are supported")
        tasks = self.NMS_TASKS.get(self.test_cfg.get("dataset"))
        if tasks is None:
            raise NotImplementedError(f"get_bboxes: no NMS task table for dataset={self.test_cfg.get('dataset')!r} "
                                      "(nuScenes, Waymo)")
        task_of_class = [-1] * self.num_classes
        for t, (classes, _) in enumerate(tasks):
            for c in classes:
                if c < self.num_classes:
                    task_of_class[c] = t
        modes = [nms_type if radius > 0 else "keep" for _, radius in tasks]
        if nms_type == "circle":
            pre, post = None, 83        # circle_nms's default post_max_size: the reference passes none
        else:
            pre, post = self.test_cfg.get("pre_maxsize"), self.test_cfg.get("post_maxsize")
        return dict(modes=modes, thresholds=[float(r) for _, r in tasks], task_of_class=task_of_class,
                    pre_maxsize=pre, post_max_size=post)

    def decode_and_nms(self, preds_dicts):
        """the device half of get_bboxes: isf_decode_boxes, then (nms_type circle / rotate) one isf_nms_segmented launch
        for the whole batch.  -> boxes [B, P, 7|9], scores [B, P], labels [B, P] int32, counts [B] int32, keep [B, P]
        bool (rows kept by the NMS; None without NMS, then rows [0, counts[b]) are the result).  No host sync."""
        assert len(preds_dicts) == 1, "one feature level"
        pd = preds_dicts[0][0]
        P, bc = self.num_proposals, self.bbox_coder
        last = {k: pd[k][..., -P:] for k in ("heatmap", "center", "height", "dim", "rot")}
        vel = pd["vel"][..., -P:] if "vel" in pd else None
        cell = [bc["out_size_factor"] * bc["voxel_size"][0], bc["out_size_factor"] * bc["voxel_size"][1]]
        boxes, scores, labels, counts = ops.decode_boxes(
            last["heatmap"], pd["query_heatmap_score"], self.query_labels, last["center"], last["height"], last["dim"],
            last["rot"], vel, cell, bc["pc_range"], bc["post_center_range"], bc["score_threshold"])
        plan = self._nms_plan()
        if plan is None:
            return boxes, scores, labels, counts, None
        from . import nms
        B = boxes.shape[0]
        keep, _, _ = nms.segmented_nms(boxes.view(B * P, -1), scores.view(-1), group_stride=P, labels=labels.view(-1),
                                       counts=counts, box_format=nms.BOX_LIDAR, **plan)
        return boxes, scores, labels, counts, keep.view(B, P)

    @torch.no_grad()
    def get_bboxes(self, preds_dicts, metas=None, img=None, rescale=False, for_roi=False):
        """:1278-1418: proposal scores, box decoding and the centre-range / score filter in one kernel
        (isf_decode_boxes); with test_cfg nms_type 'circle' / 'rotate' the per-task NMS of :1314-1403 for the whole batch
        in one more launch (isf_nms_segmented; circle_nms / nms_gpu semantics, the task table of NMS_TASKS), and the
        kept boxes compacted on the device in their decode order, as the reference's keep mask leaves them.
        -> one [boxes, scores, labels] per sample (the reference asserts a single sample, :1407-1408); boxes are wrapped
        in metas[i]['box_type_3d'] when the meta carries one.
        Deviation: the rotate branch reads test_cfg pre_maxsize / post_maxsize with .get (None when absent); the
        reference indexes them and raises KeyError with the shipped test_cfg, which has neither.  Circle NMS keeps
        circle_nms's default post_max_size=83, as the reference calls it without one."""
        boxes, scores, labels, counts, keep = self.decode_and_nms(preds_dicts)
        if keep is not None:
            B, P = keep.shape
            # stable compaction of the kept rows: row r goes to its rank among the sample's kept rows; the rest to a
            # spare row past the end
            dst = torch.cumsum(keep, 1, dtype=torch.int64) - 1
            base = torch.arange(B, device=keep.device)[:, None] * P
            dst = torch.where(keep, base + dst, torch.full_like(dst, B * P)).view(-1)
            D = boxes.shape[-1]
            cb = boxes.new_empty((B * P + 1, D)).index_copy_(0, dst, boxes.view(B * P, D))
            cs = scores.new_empty(B * P + 1).index_copy_(0, dst, scores.view(-1))
            cl = labels.new_empty(B * P + 1).index_copy_(0, dst, labels.view(-1))
            boxes, scores, labels = cb[:B * P].view(B, P, D), cs[:B * P].view(B, P), cl[:B * P].view(B, P)
            counts = keep.sum(1)
        res = []
        for i, n in enumerate(counts.tolist()):
            b = boxes[i, :n]
            box_type = (metas[i] if metas and i < len(metas) else {}).get("box_type_3d")
            res.append([box_type(b, box_dim=b.shape[-1]) if box_type is not None else b, scores[i, :n], labels[i, :n]])
        return res
