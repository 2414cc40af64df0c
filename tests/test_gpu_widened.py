"""GPU parity tests of the widened rows and of BASELINE configs[0] / [4]: box decoding
(get_bboxes), the input pre-pass, sparse-conv / MSDA / attention backward, the single-pass f16 mode, the neck on the
linear kernel, and the direct comparisons with reference-generated goldens (encoder wiring, DynamicVFE, detector).
First run on an MI355X in round 2 (profiles/r02_call1_knockout_variants.txt: 52 passed); all through the C ABI."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HEAD_KEYS = ("center", "height", "dim", "rot", "vel", "heatmap", "query_heatmap_score")


@pytest.mark.parametrize("coder", ["shipped", "tight"])
@pytest.mark.parametrize("name", ["small", "full"])
def test_get_bboxes_matches_reference_golden(dev, golden, name, coder):
    """isf_decode_boxes behind TransFusionHeadV2.get_bboxes vs the reference's get_bboxes (nms_type=None)"""
    from fusion_common import HEAD_CODERS, HEAD_CONFIGS, head_kwargs
    from isfusion_amd.transfusion_head import TransFusionHeadV2
    g = golden("head_ref.npz")
    cfg = HEAD_CONFIGS[name]
    head = TransFusionHeadV2(bbox_coder=HEAD_CODERS[coder], **head_kwargs(cfg)).eval()
    head.query_labels = torch.from_numpy(g[name + ".labels"]).to(dev)
    pd = {k: torch.from_numpy(g[f"{name}.{k}"]).to(dev) for k in HEAD_KEYS}
    res = head.get_bboxes(([pd],), [dict() for _ in range(cfg["B"])])
    assert len(res) == cfg["B"]
    for i, (boxes, scores, labels) in enumerate(res):
        ref = g[f"{name}.{coder}.{i}.boxes"]
        assert tuple(boxes.shape) == ref.shape, "kept proposals differ"
        assert labels.dtype == torch.int32
        assert np.array_equal(labels.cpu().numpy(), g[f"{name}.{coder}.{i}.box_labels"])
        assert np.abs(scores.cpu().numpy() - g[f"{name}.{coder}.{i}.scores"]).max() < 1e-6
        if ref.size:
            # expf / atan2f of the device library vs glibc: a few ulp of values up to ~60
            assert np.abs(boxes.cpu().numpy() - ref).max() < 2e-5


def test_get_bboxes_box_type_and_simple_test(dev, golden):
    """metas[i]['box_type_3d'] wraps the boxes (:1409-1417); simple_test_pts returns CPU result dicts
    (isfusion.py:274-283)"""
    from fusion_common import HEAD_CONFIGS, HEAD_SEED, head_input, head_kwargs
    from isfusion_amd.fusion_modules import seeded_state_dict
    from isfusion_amd.transfusion_head import TransFusionHeadV2
    cfg = HEAD_CONFIGS["small"]
    head = TransFusionHeadV2(**head_kwargs(cfg)).eval()
    head.load_state_dict(seeded_state_dict(head, HEAD_SEED))
    head = head.to(dev)
    outs = head(head_input(cfg).to(dev))

    class Boxes:
        def __init__(self, t, box_dim):
            self.tensor, self.box_dim = t, box_dim

    res = head.get_bboxes(outs, [dict(box_type_3d=Boxes) for _ in range(cfg["B"])])
    g = golden("head_ref.npz")
    for i, (boxes, scores, labels) in enumerate(res):
        assert isinstance(boxes, Boxes) and boxes.box_dim == 9
        ref = g[f"small.shipped.{i}.boxes"]
        assert tuple(boxes.tensor.shape) == ref.shape
        assert np.abs(boxes.tensor.cpu().numpy() - ref).max() < 2e-3      # through the HIP head forward
        assert np.abs(scores.cpu().numpy() - g[f"small.shipped.{i}.scores"]).max() < 1e-3


# ------------------------------------------------------------------------------------------- input pre-pass (8f #3)
def _as_results(key, sweeps, ts):
    return dict(pts_filename=key, timestamp=ts,
                sweeps=[dict(data_path=s["points"], timestamp=s["timestamp"],
                             sensor2lidar_rotation=s["sensor2lidar_rotation"],
                             sensor2lidar_translation=s["sensor2lidar_translation"]) for s in sweeps])


@pytest.mark.parametrize("case", ["test", "remove_close", "train_aug"])
def test_input_prepass_matches_reference_pipeline(dev, golden, case):
    """isf_assemble_points (whole batch, one call) vs the reference's per-sample CPU pipeline"""
    from input_common import INPUT_CONFIGS, PC_RANGE, sweep_inputs, train_aug
    from isfusion_amd.input_pipeline import MultiSweepPointLoader
    g = golden("input_ref.npz")
    names = ["a", "b", "key_only"]
    batch = [_as_results(*sweep_inputs(*INPUT_CONFIGS[n])) for n in names]
    loader = MultiSweepPointLoader(sweeps_num=10, remove_close=(case == "remove_close"), test_mode=True,
                                   point_cloud_range=PC_RANGE, device=dev)
    aug = [train_aug(77) for _ in names] if case == "train_aug" else None
    out = loader(batch, aug=aug)
    assert len(out) == len(names)
    for n, pts in zip(names, out):
        ref = g[f"{n}.{case}.points"]
        assert tuple(pts.shape) == ref.shape, f"{n}: kept {pts.shape[0]} points, reference {ref.shape[0]}"
        got = pts.cpu().numpy()
        if case == "train_aug":
            # the float32 [P,3]x[3,3] rotation's summation order / FMA use is the BLAS's choice: a few ulp (7.6e-6 at
            # |coord| up to 79) carried through translate and scale; no point is closer than 3.7e-4 to a range bound
            assert np.abs(got - ref).max() < 6e-5
        else:
            # float64 pose arithmetic rounded to float32: bit-exact up to fused-multiply-add double rounding
            assert np.abs(got - ref).max() <= 4e-6
            assert (got != ref).mean() < 1e-3
        assert np.array_equal(got[:, 3], ref[:, 3])


def test_input_prepass_feeds_the_lidar_branch(dev):
    """pre-pass output == oracle pipeline output, handed to the voxelizer as the reference's collate would"""
    from input_common import INPUT_CONFIGS, PC_RANGE, sweep_inputs
    from isfusion_amd.input_pipeline import MultiSweepPointLoader
    from oracle import input_ops
    key, sweeps, ts = sweep_inputs(*INPUT_CONFIGS["a"])
    loader = MultiSweepPointLoader(test_mode=True, point_cloud_range=PC_RANGE, device=dev)
    pts = loader([_as_results(key, sweeps, ts)] * 2)
    ref = input_ops.load_frame(key, sweeps, ts, PC_RANGE)
    for p in pts:
        assert tuple(p.shape) == ref.shape and np.abs(p.cpu().numpy() - ref).max() <= 4e-6
    # empty sweep list and an empty file
    empty = loader([dict(pts_filename=np.zeros((0, 5), np.float32), timestamp=ts, sweeps=[])])
    assert empty[0].shape == (0, 5)


@pytest.mark.parametrize("with_aug", [False, True])
def test_input_prepass_block_count_multiple_of_64(dev, with_aug):
    """the block-offset scan writes n + 1 entries: with a total block count that is a multiple of 64 the extra word
    used to land in the next arena allocation (the augmentation table / the scan's own partial sums).  30 + 17 + 17
    workgroups of 256 points = 64 blocks; several samples so that per-sample offsets are exercised too."""
    from input_common import PC_RANGE, sweep_inputs, train_aug
    from isfusion_amd.input_pipeline import MultiSweepPointLoader
    from oracle import input_ops
    frames = [sweep_inputs(21, 256 * 30, (256 * 17, 256 * 17)), sweep_inputs(22, 256 * 40, (256 * 24,)),
              sweep_inputs(23, 256 * 64, ())]
    loader = MultiSweepPointLoader(test_mode=True, point_cloud_range=PC_RANGE, device=dev)
    for group in ([0], [0, 1], [1, 2], [0, 1, 2]):           # 64, 128, 128, 192 blocks
        aug = [train_aug(90 + i) if (with_aug and i != 1) else None for i in group] if with_aug else None
        out = loader([_as_results(*frames[i]) for i in group], aug=aug)
        for j, i in enumerate(group):
            ref = input_ops.load_frame(*frames[i], PC_RANGE, aug=aug[j] if aug else None)
            assert tuple(out[j].shape) == ref.shape, (group, i, out[j].shape, ref.shape)
            assert np.abs(out[j].cpu().numpy() - ref).max() < (6e-5 if with_aug else 4e-6)


# ------------------------------------------------------------------------------------------- BASELINE configs[0], [4]
VS = [0.075, 0.075, 0.2]
RG = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_baseline_config0_hard_vfe_three_stage_encoder(dev, oracle_mod):
    """BASELINE configs[0] (the reference's CPU-runnable case): one 20k-point cloud, 0.075 m hard voxelization,
    HardSimpleVFE, 3-stage sparse encoder -> BEV, HIP vs the C oracle composition.  1e-3 on BEV features."""
    import isfusion_amd as m
    from isfusion_amd import synthetic
    pts = synthetic.lidar_sweeps(2020, 20000)
    me = dict(in_channels=5, sparse_shape=[41, 1440, 1440], output_channels=32,
              encoder_channels=((16,), (32,), (64,)), encoder_paddings=((1,), (1,), (1,)))
    lb = m.LidarBranch(pts_middle_encoder=me).randomize_weights_(3).randomize_bn_(4).eval().to(dev)
    enc = lb.pts_middle_encoder
    v, c, n = m.voxelization(_T(pts, dev), VS, RG, 10, 60000)
    ov, oc, on = oracle_mod.hard_voxelize(pts, VS, RG, 10, 60000)
    assert np.array_equal(c.cpu().numpy(), oc) and np.array_equal(n.cpu().numpy(), on)
    assert np.array_equal(v.cpu().numpy(), ov)
    vf = m.HardSimpleVFE(num_features=5)(v, n, c)
    ovf = oracle_mod.hard_simple_vfe(ov, on, 5)
    assert np.abs(vf.cpu().numpy() - ovf).max() < 1e-5
    c4 = torch.cat([torch.zeros((c.shape[0], 1), dtype=c.dtype, device=dev), c], 1)
    bev = enc.forward_fused(vf, c4, 1)
    obev, outs = oracle_mod.sparse_encoder_forward(enc.plan_to_numpy(), ovf,
                                                   np.concatenate([np.zeros((len(oc), 1), np.int32), oc], 1), 1)
    assert tuple(bev.shape) == obev.shape
    assert np.abs(bev.cpu().numpy() - obev).max() < 1e-3
    assert np.array_equal(bev.cpu().numpy() != 0, obev != 0) and np.abs(obev).max() > 0.1


def test_baseline_config4_stress_005_voxels(dev, oracle_mod):
    """BASELINE configs[4]: 0.05 m voxels (sparse shape [41, 2160, 2160]), 500k points per frame.  Oracle parity at a
    size the scalar oracle finishes in seconds, then size-independent properties at full size."""
    import isfusion_amd as m
    from isfusion_amd import synthetic
    from isfusion_amd.norm import fold_bn
    from isfusion_amd.voxelize import dynamic_voxelize_batched
    vs = [0.05, 0.05, 0.2]
    me = dict(m.ISFUSION_0075["pts_middle_encoder"])
    me["sparse_shape"] = [41, 2160, 2160]
    lb = m.LidarBranch(voxel_size=vs, pts_middle_encoder=me).randomize_weights_(0).randomize_bn_(1).eval()
    # ---- small: vs oracle
    B = 2
    pl = [synthetic.lidar_sweeps(900 + i, 4000) for i in range(B)]
    coors = np.concatenate([np.concatenate([np.full((p.shape[0], 1), b, np.int32),
                                            oracle_mod.dynamic_voxelize(p, vs, RG)], 1) for b, p in enumerate(pl)])
    vfe = lb.pts_voxel_encoder
    bn1 = [t.numpy() for t in fold_bn(vfe.vfe_layers[0].norm)]
    bn2 = [t.numpy() for t in fold_bn(vfe.vfe_layers[1].norm)]
    ovf, ovc, _ = oracle_mod.dynamic_vfe(np.concatenate(pl), coors, vs, RG,
                                         vfe.vfe_layers[0].linear.weight.detach().numpy(), bn1,
                                         vfe.vfe_layers[1].linear.weight.detach().numpy(), bn2)
    obev, _ = oracle_mod.sparse_encoder_forward(lb.pts_middle_encoder.plan_to_numpy(), ovf, ovc, B)
    lb = lb.to(dev)
    out = lb([_T(p, dev) for p in pl])
    assert tuple(out.shape) == obev.shape == (B, 512, 270, 270)
    assert np.abs(out.cpu().numpy() - obev).max() < 1e-3
    # ---- full size: properties
    P = 500000
    big = [_T(synthetic.lidar_sweeps(7000 + i, P), dev) for i in range(B)]
    o1 = lb(big, want_stats=True)
    st = lb.last_stats
    assert torch.isfinite(o1).all() and tuple(o1.shape) == (B, 512, 270, 270)
    _, cc = dynamic_voxelize_batched(big, vs, RG)
    assert st.num_in[0] == torch.unique(cc[(cc[:, 1:] >= 0).all(1)], dim=0).shape[0]
    assert torch.equal(o1, lb(big)), "not deterministic"
    assert torch.equal(lb([big[1]])[0], o1[1]), "frames are not independent"


def test_baseline_config4_stress_005_voxels_f16_storage(dev):
    """BASELINE configs[4] in ITS OWN data type at ITS OWN size: 0.05 m voxels, 500 k points per frame, f16 storage
    (isf_encoder_options.precision = 2: f16 rows between the layers, f16 operands, fp32 accumulate -- the reference's
    indice_conv_half).  Size-independent properties at full size: determinism, frame independence (a frame alone == the
    same frame in a batch, bit for bit), the same occupied BEV cells as the fp32-class run, and agreement with it to f16
    tolerance after 21 layers (one f16 ulp per layer op on O(1) features: a few 1e-3 of the feature scale)."""
    import isfusion_amd as m
    from isfusion_amd import synthetic
    vs = [0.05, 0.05, 0.2]
    me = dict(m.ISFUSION_0075["pts_middle_encoder"])
    me["sparse_shape"] = [41, 2160, 2160]
    lb = m.LidarBranch(voxel_size=vs, pts_middle_encoder=me).randomize_weights_(0).randomize_bn_(1).eval().to(dev)
    B, P = 2, 500000
    big = [_T(synthetic.lidar_sweeps(7100 + i, P), dev) for i in range(B)]
    h1 = lb(big, precision=2, want_stats=True)
    assert lb.last_stats.num_in[0] > 300000                       # 2 x ~170 k voxels: the 0.05 m grid is the stress case
    assert torch.isfinite(h1).all() and tuple(h1.shape) == (B, 512, 270, 270)
    assert torch.equal(h1, lb(big, precision=2)), "f16 storage: not deterministic"
    assert torch.equal(lb([big[1]], precision=2)[0], h1[1]), "f16 storage: frames are not independent"
    f1 = lb(big)                                                  # fp32-class arithmetic on the same frames
    scale = f1.abs().max().item()
    assert scale > 0.1
    # the occupied cells are geometry, not arithmetic: identical up to ReLU flips of values that are ~0 on both sides
    differ = (h1 != 0) != (f1 != 0)
    assert (torch.maximum(h1.abs(), f1.abs())[differ] < 3e-2 * scale).all()
    err = (h1 - f1).abs().max().item()
    assert err < 3e-2 * scale, (err, scale)                       # f16 tolerance after 21 layers (as the small-size test)
    assert (h1 - f1).abs().mean().item() < 3e-3 * scale


@pytest.mark.parametrize("name,seed,P,nf", [("nf4", 31, 3000, 4), ("nf5", 32, 2500, 5)])
def test_hard_simple_vfe_matches_reference_golden(dev, golden, oracle_mod, name, seed, P, nf):
    import isfusion_amd as m
    from isfusion_amd import synthetic
    v, c, n = oracle_mod.hard_voxelize(synthetic.lidar_sweeps(seed, P), VS, RG, 10, 20000)
    out = m.HardSimpleVFE(num_features=nf)(_T(v, dev), _T(n, dev), _T(c, dev))
    ref = golden("vfe_ref.npz")[name]
    assert tuple(out.shape) == ref.shape and np.abs(out.cpu().numpy() - ref).max() < 1e-5


# ------------------------------------------------------------------------------------------- conv backward (8f #2)
@pytest.mark.parametrize("case", ["subm_k3", "conv_s2p1", "conv_s2p011", "conv_311", "subm_5to16"])
def test_sparse_conv_backward_vs_oracle_golden_geometries(dev, golden, oracle_mod, case):
    """SparseConvFunction.backward (isf_sparse_conv_backward_input / _filter) vs the C restatement of
    indice_conv_backward (itself pinned to conv3d autograd) on the golden rulebook geometries"""
    import isfusion_amd as m
    from isfusion_amd import spconv
    g = golden("spconv_dense_ref.npz")
    cfg = g[case + "_cfg"]
    B, shape, ks, st, pd, subm = int(cfg[0]), [int(v) for v in cfg[1:4]], [int(v) for v in cfg[4:7]], \
        [int(v) for v in cfg[7:10]], [int(v) for v in cfg[10:13]], bool(cfg[13])
    idx, feats, w = g[case + "_idx"], g[case + "_feats"], g[case + "_w"]
    # the library orders rows (b,z,y,x): feed sorted rows so that gradients line up with the oracle's
    order = np.lexsort((idx[:, 3], idx[:, 2], idx[:, 1], idx[:, 0]))
    idx, feats = idx[order], feats[order]
    out_idx, pairs, num = oracle_mod.get_indice_pairs(idx, B, shape, ks, st, pd, subm=subm)
    cls = m.SubMConv3d if subm else m.SparseConv3d
    conv = cls(w.shape[-2], w.shape[-1], ks, stride=st, padding=pd, bias=True).to(dev)
    with torch.no_grad():
        conv.weight.copy_(_T(w, dev))
    x = _T(feats, dev).requires_grad_()
    assert spconv.TRAINING_KERNELS          # the default since the backward kernels were validated on hardware
    out = conv(m.SparseConvTensor(x, _T(idx, dev), shape, B))
    # rows of the strided output are sorted (b,z,y,x); the oracle numbers them first-come
    oi = out.indices.cpu().numpy()
    key = {tuple(r): i for i, r in enumerate(out_idx.tolist())}
    perm = np.array([key[tuple(r)] for r in oi.tolist()])
    gout = np.random.default_rng(5).normal(size=(out_idx.shape[0], w.shape[-1])).astype(np.float32)
    out.features.backward(_T(gout[perm], dev))
    y = oracle_mod.indice_conv(feats, w, pairs, num, out_idx.shape[0])
    assert np.abs(out.features.detach().cpu().numpy() - (y[perm] + conv.bias.detach().cpu().numpy())).max() < 2e-4
    dx, dw = oracle_mod.indice_conv_backward(feats, w, gout, pairs, num)
    assert np.abs(x.grad.cpu().numpy() - dx).max() < 2e-4
    assert np.abs(conv.weight.grad.cpu().numpy() - dw).max() < 2e-4 * max(1.0, np.abs(dw).max())
    assert np.abs(conv.bias.grad.cpu().numpy() - gout.sum(0)).max() < 1e-3


@pytest.mark.parametrize("gscale", [1.0, 1e-6])
@pytest.mark.parametrize("cin,cout", [(16, 16), (32, 64), (64, 64), (128, 64), (128, 256), (256, 256)])
def test_sparse_conv_backward_channel_shapes(dev, oracle_mod, cin, cout, gscale):
    """every (Cin, Cout) block shape of the dW kernel and the transposed-filter dX path; several row chunks; gradients
    of O(1) and of the size a real backward pass carries (1e-6)"""
    from isfusion_amd import spconv
    rng = np.random.default_rng(cin * 1000 + cout)
    B, shape = 2, [9, 24, 24]
    n = 1500
    cells = rng.choice(B * shape[0] * shape[1] * shape[2], n, replace=False)
    cells.sort()
    idx = np.stack(np.unravel_index(cells, (B, *shape)), 1).astype(np.int32)
    feats = rng.normal(size=(n, cin)).astype(np.float32)
    w = (rng.normal(size=(3, 3, 3, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32)
    out_idx, pairs, num = oracle_mod.get_indice_pairs(idx, B, shape, [3, 3, 3], [1, 1, 1], [1, 1, 1], subm=True)
    gout = (rng.normal(size=(n, cout)) * gscale).astype(np.float32)
    dx, dw = oracle_mod.indice_conv_backward(feats, w, gout, pairs, num)
    rb = spconv.build_rulebook(_T(idx, dev), B, shape, [3, 3, 3], [1, 1, 1], [1, 1, 1], True)
    x, wt = _T(feats, dev).requires_grad_(), _T(w, dev).requires_grad_()
    out = spconv.SparseConvFunction.apply(x, wt, rb)
    out.backward(_T(gout, dev))
    assert np.abs(x.grad.cpu().numpy() - dx).max() < 1e-3 * max(gscale, np.abs(dx).max())
    assert np.abs(wt.grad.cpu().numpy() - dw).max() < 1e-3 * max(gscale, np.abs(dw).max())
    # deterministic: a second backward gives the same bits
    x2, w2 = _T(feats, dev).requires_grad_(), _T(w, dev).requires_grad_()
    spconv.SparseConvFunction.apply(x2, w2, rb).backward(_T(gout, dev))
    assert torch.equal(x.grad, x2.grad) and torch.equal(wt.grad, w2.grad)


def test_pair_lists_equal_the_interchange_format_and_its_counts(dev):
    """isf_rulebook_pair_lists (two-pass ordered compaction, round 5) == isf_rulebook_to_indice_pairs (one workgroup per
    tap): same pairs in the same order, same counts, -1 padding behind them; SubM and strided rulebooks, a level larger
    than one 2048-row block and an empty one"""
    from isfusion_amd import _lib, spconv
    lib = _lib.load()
    rng = np.random.default_rng(11)
    B, shape = 2, [12, 40, 40]
    for n, subm in ((9000, True), (9000, False), (700, True), (0, True)):
        cells = np.sort(rng.choice(B * int(np.prod(shape)), n, replace=False))
        idx = np.stack(np.unravel_index(cells, (B, *shape)), 1).astype(np.int32).reshape(-1, 4)
        if n == 0:
            continue   # build_rulebook of an empty tensor is covered elsewhere; the C entry's num_out == 0 path below
        rb = spconv.build_rulebook(_T(idx, dev), B, shape, [3, 3, 3], [1, 1, 1] if subm else [2, 2, 2], [1, 1, 1], subm)
        K = rb.nbr.numel() // rb.stride
        pairs, num, cap = spconv.pair_lists(rb)
        ref_pairs = torch.full((K, 2, max(rb.num_in, 1)), -7, dtype=torch.int32, device=dev)
        ref_num = torch.zeros(K, dtype=torch.int32, device=dev)
        _lib.check(lib.isf_rulebook_to_indice_pairs(_lib.ptr(rb.nbr), rb.stride, rb.num_out, K, rb.num_in, _lib.ptr(ref_pairs),
                                                    _lib.ptr(ref_num), _lib.stream()))
        assert torch.equal(num, ref_num)
        assert cap % 32 == 0 and cap >= int(num.max()) + 32
        for k in range(K):
            c = int(num[k])
            assert torch.equal(pairs[k, :, :c], ref_pairs[k, :, :c]), (n, subm, k)
            assert (pairs[k, :, c:c + 32] == -1).all()
    num = torch.full((27,), 5, dtype=torch.int32, device=dev)
    pairs = torch.zeros((27, 2, 32), dtype=torch.int32, device=dev)
    nbr = torch.zeros((27 * 128,), dtype=torch.int32, device=dev)
    _lib.check(lib.isf_rulebook_pair_lists(_lib.ptr(nbr), 128, 0, 27, 32, _lib.ptr(pairs), _lib.ptr(num), _lib.stream()))
    assert int(num.abs().sum()) == 0 and (pairs == -1).all()


@pytest.mark.parametrize("cin,cout,n,subm", [(32, 32, 30000, True), (64, 32, 12000, True), (32, 64, 12000, False),
                                            (64, 64, 30000, True), (128, 128, 9000, True), (128, 256, 9000, False),
                                            (256, 256, 6000, True), (256, 128, 777, True)])
def test_wgrad_f16x3_matches_fp64_and_the_fp32_mfma_kernel(dev, cin, cout, n, subm):
    """isf_sparse_conv_backward_filter_f16x3 (round 5: dW on v_mfma_f32_16x16x32_f16 in the f16x3 split, pair lists,
    LDS-transposed staging) against a float64 sum over the pairs and against the fp32-MFMA kernel it replaces: every
    block shape, several pair chunks per tap, taps with zero / ragged pair counts, strided rulebooks (num_in != num_out),
    gradients of the size a real backward carries; deterministic"""
    from isfusion_amd import _lib, spconv
    lib = _lib.load()
    rng = np.random.default_rng(cin + 7 * cout + n)
    B, shape = 2, [10, 48, 48]
    cells = np.sort(rng.choice(B * int(np.prod(shape)), n, replace=False))
    idx = np.stack(np.unravel_index(cells, (B, *shape)), 1).astype(np.int32)
    rb = spconv.build_rulebook(_T(idx, dev), B, shape, [3, 3, 3], [1, 1, 1] if subm else [2, 2, 2], [1, 1, 1], subm)
    K = 27
    x = torch.randn(rb.num_in, cin, device=dev) * 0.7
    g = torch.randn(rb.num_out, cout, device=dev) * 3e-7
    g[::17] *= 40.0                                     # a few large rows set the scale
    xs = spconv.to_split(x)
    gs, sc = spconv.grad_to_split(g)
    s = float(sc[0])
    assert s == 2.0 ** round(np.log2(s)) and 2 ** 9 <= float(g.abs().max()) * s < 2 ** 10
    assert abs(float(sc[1]) * s - 1.0) < 1e-6
    got = spconv.sparse_conv_backward_filter_f16x3(xs, cin, gs, cout, rb, sc[1:], (3, 3, 3, cin, cout)).view(K, cin, cout)
    again = spconv.sparse_conv_backward_filter_f16x3(xs, cin, gs, cout, rb, sc[1:], (3, 3, 3, cin, cout)).view(K, cin, cout)
    assert torch.equal(got, again)
    old = torch.empty(K, cin, cout, device=dev)
    _lib.check(lib.isf_sparse_conv_backward_filter(_lib.ptr(x), rb.num_in, cin, _lib.ptr(g), rb.num_out, cout,
                                                   _lib.ptr(rb.nbr), rb.stride, K, _lib.ptr(old), _lib.stream()))
    nbr = rb.nbr.view(K, rb.stride)[:, :rb.num_out]
    x64, g64 = x.double(), g.double()
    want = torch.zeros(K, cin, cout, dtype=torch.float64, device=dev)
    for k in range(K):
        o = torch.nonzero(nbr[k] >= 0).flatten()
        if o.numel():
            want[k] = x64[nbr[k][o].long()].T @ g64[o]
    scale = float(want.abs().max())
    assert scale > 0
    assert float((got.double() - want).abs().max()) < 2e-5 * scale, float((got.double() - want).abs().max()) / scale
    assert float((old.double() - want).abs().max()) < 2e-5 * scale


@pytest.mark.parametrize("cin,cout,subm", [(32, 32, True), (64, 128, False), (128, 128, True), (256, 256, True)])
def test_sparse_conv_half_mode_is_the_references_autocast_arithmetic(dev, cin, cout, subm):
    """SparseConvFunction(half=True) -- what SparseConvolution.forward selects under torch.autocast, as the reference's
    custom_fwd(cast_inputs=torch.half) does: fp16 operands (the hi halves only), fp32 accumulation, in forward, dX and dW.
    Against float64 on f16-ROUNDED operands the three results are fp32-accurate (the rounding of the operands is the whole
    difference to the fp32-class mode); against the unrounded float64 result they sit within fp16's 2^-11 operand error."""
    from isfusion_amd import spconv
    rng = np.random.default_rng(cin + cout)
    B, shape, n = 2, [10, 40, 40], 6000
    cells = np.sort(rng.choice(B * int(np.prod(shape)), n, replace=False))
    idx = np.stack(np.unravel_index(cells, (B, *shape)), 1).astype(np.int32)
    rb = spconv.build_rulebook(_T(idx, dev), B, shape, [3, 3, 3], [1, 1, 1] if subm else [2, 2, 2], [1, 1, 1], subm)
    K = 27
    x = torch.randn(rb.num_in, cin, device=dev)
    w = torch.randn(3, 3, 3, cin, cout, device=dev) / np.sqrt(9 * cin)
    g = torch.randn(rb.num_out, cout, device=dev) * 1e-6
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    out = spconv.SparseConvFunction.apply(xr, wr, rb, True)
    out.backward(g)
    nbr = rb.nbr.view(K, rb.stride)[:, :rb.num_out].long()

    def ref(xq, wq, gq):
        y = torch.zeros(rb.num_out, cout, dtype=torch.float64, device=dev)
        dx = torch.zeros(rb.num_in, cin, dtype=torch.float64, device=dev)
        dw = torch.zeros(K, cin, cout, dtype=torch.float64, device=dev)
        wk = wq.view(K, cin, cout)
        for k in range(K):
            o = torch.nonzero(nbr[k] >= 0).flatten()
            if o.numel():
                i = nbr[k][o]
                y[o] += xq[i] @ wk[k]
                dx.index_add_(0, i, gq[o] @ wk[k].T)
                dw[k] = xq[i].T @ gq[o]
        return y, dx, dw
    # the kernels scale weights / gradients by a power of two before rounding to f16: rounding commutes with it
    sw = 2.0 ** (12 - np.ceil(np.log2(float(w.abs().max()))))
    sg = float(spconv.grad_to_split(g)[1][0])
    h = lambda t, s=1.0: ((t * s).half().double() / s)
    ya, dxa, dwa = ref(h(x), h(w, sw), h(g, sg))
    for got, want in ((out, ya), (xr.grad, dxa), (wr.grad.view(K, cin, cout), dwa)):
        assert float((got.double() - want).abs().max()) < 3e-5 * float(want.abs().max())
    yb, dxb, dwb = ref(x.double(), w.double(), g.double())
    for got, want in ((out, yb), (xr.grad, dxb), (wr.grad.view(K, cin, cout), dwb)):
        e = float((got.double() - want).abs().max()) / float(want.abs().max())
        assert 1e-7 < e < 5e-3, e            # NOT the fp32-class path: fp16 operand rounding is visible, and bounded


def test_sparse_conv_modules_use_the_half_kernels_under_autocast_only(dev):
    """SubMConv3d.forward in training mode: fp32-class arithmetic by default, the half kernels under torch.autocast (the
    reference's custom_fwd(cast_inputs=torch.half)), and fp32-class again with spconv.AUTOCAST_HALF = False"""
    import isfusion_amd as m
    from isfusion_amd import spconv
    rng = np.random.default_rng(5)
    B, shape, n, c = 2, [9, 24, 24], 2500, 64
    cells = np.sort(rng.choice(B * int(np.prod(shape)), n, replace=False))
    idx = _T(np.stack(np.unravel_index(cells, (B, *shape)), 1).astype(np.int32), dev)
    conv = m.SubMConv3d(c, c, 3, padding=1, bias=False).to(dev).train()
    x = torch.randn(n, c, device=dev)

    def run():
        return conv(m.SparseConvTensor(x, idx, shape, B)).features.detach()
    full = run()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        half = run()
        assert half.dtype == torch.float32
        spconv.AUTOCAST_HALF = False
        try:
            full2 = run()
        finally:
            spconv.AUTOCAST_HALF = True
    assert torch.equal(full, full2)
    e = float((half - full).abs().max()) / float(full.abs().max())
    assert 1e-6 < e < 5e-3, e


def test_training_path_without_the_f16_wgrad_still_works(dev):
    """spconv.WGRAD_F16X3 = False restores the round-2 backward (fp32-MFMA dW, torch-op gradient scaling); both paths
    agree to fp32 rounding.  Its dX runs on the rulebook's cached transposed view: a second call reuses the view and the
    tile order built on it, and gives the same bits."""
    from isfusion_amd import spconv
    rng = np.random.default_rng(3)
    B, shape, n, cin, cout = 2, [9, 24, 24], 1500, 64, 128
    cells = np.sort(rng.choice(B * int(np.prod(shape)), n, replace=False))
    idx = np.stack(np.unravel_index(cells, (B, *shape)), 1).astype(np.int32)
    rb = spconv.build_rulebook(_T(idx, dev), B, shape, [3, 3, 3], [1, 1, 1], [1, 1, 1], True)
    feats = torch.randn(n, cin, device=dev)
    w = torch.randn(3, 3, 3, cin, cout, device=dev) / np.sqrt(27 * cin)
    gout = torch.randn(n, cout, device=dev) * 1e-6
    res = []
    try:
        for flag in (True, False, False):
            spconv.WGRAD_F16X3 = flag
            x, wt = feats.clone().requires_grad_(), w.clone().requires_grad_()
            out = spconv.SparseConvFunction.apply(x, wt, rb)
            out.backward(gout)
            res.append((out.detach(), x.grad, wt.grad, rb.transposed(), dict(rb.transposed().derived)))
    finally:
        spconv.WGRAD_F16X3 = True
    assert torch.equal(res[0][0], res[1][0])
    for a, b in zip(res[0][1:3], res[1][1:3]):
        assert float((a - b).abs().max()) < 1e-4 * float(b.abs().max())
    assert res[0][3] is res[1][3] is res[2][3] and (res[0][3].num_in, res[0][3].num_out) == (rb.num_out, rb.num_in)
    # the split path launches in launch order and builds nothing; the cross-check's dX builds one tile order (128 -> 64), once
    assert res[0][4] == {} and list(res[1][4]) == [("tile_order", cout, cin, 0)] and res[2][4].keys() == res[1][4].keys()
    assert all(res[2][4][k] is v for k, v in res[1][4].items())
    assert all(torch.equal(a, b) for a, b in zip(res[1][:3], res[2][:3]))


def test_sparse_encoder_training_step_matches_torch_dense_autograd(dev):
    """SparseEncoder in train() mode (module-by-module: HIP conv Function + stock BatchNorm1d / ReLU, as the reference
    composes them) -- loss.backward() vs the same network written with dense torch conv3d on the zero-filled grid
    restricted to the active sites (valid for SubM stacks: here conv_input + one SubM stage)."""
    import isfusion_amd as m
    from isfusion_amd import spconv
    rng = np.random.default_rng(8)
    B, shape, n, cin = 2, [8, 16, 16], 600, 16
    cells = np.sort(rng.choice(B * shape[0] * shape[1] * shape[2], n, replace=False))
    idx = np.stack(np.unravel_index(cells, (B, *shape)), 1).astype(np.int32)
    feats = rng.normal(size=(n, cin)).astype(np.float32)
    convs = [m.SubMConv3d(cin, 32, 3, padding=1, bias=False, indice_key="subm1").to(dev),
             m.SubMConv3d(32, 32, 3, padding=1, bias=False, indice_key="subm1").to(dev)]
    bns = [torch.nn.BatchNorm1d(32, eps=1e-3, momentum=0.01).to(dev) for _ in convs]
    x = _T(feats, dev).requires_grad_()
    assert spconv.TRAINING_KERNELS
    t = m.SparseConvTensor(x, _T(idx, dev), shape, B)
    for conv, bn in zip(convs, bns):
        t = conv(t)
        t.features = torch.relu(bn(t.features))
    dense = t.dense()
    loss = (dense ** 2).mean()
    loss.backward()
    # dense torch reference on the same parameters
    ii = _T(idx, dev).long()
    xr = _T(feats, dev).requires_grad_()
    mask = torch.zeros((B, 1, *shape), device=dev)
    mask[ii[:, 0], 0, ii[:, 1], ii[:, 2], ii[:, 3]] = 1
    cur = torch.zeros((B, *shape, cin), device=dev).index_put((ii[:, 0], ii[:, 1], ii[:, 2], ii[:, 3]), xr)
    cur = cur.permute(0, 4, 1, 2, 3)
    grads_ref = []
    for conv, bn in zip(convs, bns):
        w = conv.weight.detach().clone().requires_grad_()
        grads_ref.append(w)
        y = torch.nn.functional.conv3d(cur, w.permute(4, 3, 0, 1, 2), padding=1)
        rows = y[ii[:, 0], :, ii[:, 1], ii[:, 2], ii[:, 3]]                        # active sites only (SubM)
        mu, var = rows.mean(0), rows.var(0, unbiased=False)
        rows = torch.relu((rows - mu) / torch.sqrt(var + 1e-3) * bn.weight.detach() + bn.bias.detach())
        cur = torch.zeros((B, *shape, rows.shape[1]), device=dev).index_put(
            (ii[:, 0], ii[:, 1], ii[:, 2], ii[:, 3]), rows).permute(0, 4, 1, 2, 3)
    loss_ref = (cur ** 2).mean()
    loss_ref.backward()
    assert abs(loss.item() - loss_ref.item()) < 1e-5 * max(1.0, abs(loss_ref.item()))
    assert (x.grad - xr.grad).abs().max().item() < 1e-4 * max(1.0, xr.grad.abs().max().item())
    for conv, w in zip(convs, grads_ref):
        assert (conv.weight.grad - w.grad).abs().max().item() < 1e-4 * max(1.0, w.grad.abs().max().item())


def test_sparse_encoder_training_step_shares_one_transposed_view_and_pair_list_per_rulebook(dev, monkeypatch):
    """two SubM 32 -> 32 layers on one indice_key + one strided 32 -> 64 conv, one forward and backward: both SubM layers'
    dX runs on the SAME Rulebook.transposed() object, the level's rulebook caches exactly one transposed table and one
    pair list, and the strided layer's rulebook holds its own pair of them"""
    import isfusion_amd as m
    from isfusion_amd import spconv
    rng = np.random.default_rng(18)
    B, shape, n = 1, [8, 16, 16], 300
    cells = np.sort(rng.choice(B * int(np.prod(shape)), n, replace=False))
    idx = np.stack(np.unravel_index(cells, (B, *shape)), 1).astype(np.int32)
    convs = [m.SubMConv3d(32, 32, 3, padding=1, bias=False, indice_key="subm1").to(dev),
             m.SubMConv3d(32, 32, 3, padding=1, bias=False, indice_key="subm1").to(dev),
             m.SparseConv3d(32, 64, 3, stride=2, padding=1, bias=False, indice_key="down").to(dev)]
    seen = []

    def recording(xs, packed16, K, c_in, c_out, rb, *a, _split=spconv.sparse_conv_split, **k):
        seen.append(rb)
        return _split(xs, packed16, K, c_in, c_out, rb, *a, **k)
    monkeypatch.setattr(spconv, "sparse_conv_split", recording)
    x = _T(rng.normal(size=(n, 32)).astype(np.float32), dev).requires_grad_()
    t = m.SparseConvTensor(x, _T(idx, dev), shape, B)
    for conv in convs:
        t = conv(t)
    t.features.square().mean().backward()
    level, down = t.indice_dict["subm1"], t.indice_dict["down"]
    assert level is not down and down.num_out == t.features.shape[0] > 0
    assert len(seen) == 6 and all(a is b for a, b in zip(seen, (level, level, down, down.transposed(), level.transposed(),
                                                                level.transposed())))
    for rb in (level, down):
        assert set(rb.derived) == {"transposed", "pairs"}
        assert rb.transposed().nbr is spconv.transposed_nbr(rb)[0] and rb.transposed().derived == {}
        assert (rb.transposed().num_in, rb.transposed().num_out) == (rb.num_out, rb.num_in)
    assert level.transposed() is not down.transposed() and level.derived["pairs"] is not down.derived["pairs"]
    assert float(x.grad.abs().max()) > 0 and all(float(c.weight.grad.abs().max()) > 0 for c in convs)


# ------------------------------------------------------------------------------------------- MSDA backward (8f #2)
@pytest.mark.parametrize("name,B,Q,H", [("small", 1, 20, 12), ("edge", 2, 16, 7)])
def test_msda_backward_matches_reference_autograd_golden(dev, golden, name, B, Q, H):
    """isf_msda_backward (through MSDAFunction) vs autograd through the reference's pure-torch MSDA"""
    from fusion_common import msda_grad_inputs
    from isfusion_amd import fusion_ops as ops
    g = golden("msda_grad_ref.npz")
    value, loc, aw, gout, ref, off, logits = msda_grad_inputs(B, Q, H, raw=True)
    v = value.reshape(B, H * H, 128).to(dev).requires_grad_()
    o, lg = off.to(dev).requires_grad_(), logits.to(dev).requires_grad_()
    out = ops.MSDAFunction.apply(v, o, lg, ref.to(dev), B, Q, 8, 16, 16, H, H)
    assert np.abs(out.detach().cpu().numpy() - g[name + ".out"].reshape(B * Q, 128)).max() < 5e-5
    out.backward(gout.reshape(B * Q, 128).to(dev))
    gv = g[name + ".grad_value"].reshape(B, H * H, 128)
    assert np.abs(v.grad.cpu().numpy() - gv).max() < 1e-4 * max(1.0, np.abs(gv).max())
    # loc = ref + off / (W, H)  =>  d/d off = d/d loc / (W, H)
    goff = g[name + ".grad_loc"].reshape(B * Q, 8 * 16 * 2) / H
    assert np.abs(o.grad.cpu().numpy() - goff).max() < 1e-4 * max(1.0, np.abs(goff).max())
    # attention weights = softmax(logits)
    gw = torch.from_numpy(g[name + ".grad_weight"]).reshape(B * Q, 8, 16)
    a = aw.reshape(B * Q, 8, 16)
    glog = (a * (gw - (a * gw).sum(-1, keepdim=True))).reshape(B * Q, 128).numpy()
    assert np.abs(lg.grad.cpu().numpy() - glog).max() < 1e-4 * max(1.0, np.abs(glog).max())


# ------------------------------------------------------------------------------------------- attention backward (8f #2)
def _torch_mha_core(q, k, v, B, Lq, Lk, heads):
    """softmax(q k^T / sqrt(hd)) v per head in float64 (what nn.MultiheadAttention computes after its projections)"""
    E = q.shape[1]
    hd = E // heads
    qh = q.view(B, Lq, heads, hd).transpose(1, 2)
    kh = k.view(B, Lk, heads, hd).transpose(1, 2)
    vh = v.view(B, Lk, heads, hd).transpose(1, 2)
    p = (qh @ kh.transpose(-1, -2) / hd ** 0.5).softmax(-1)
    return (p @ vh).transpose(1, 2).reshape(B * Lq, E)


@pytest.mark.parametrize("B,Lq,Lk", [(2, 50, 37), (1, 300, 200), (1, 70, 1500), (2, 5000, 200), (1, 32400, 200)])
def test_attention_backward_matches_torch_autograd(dev, B, Lq, Lk):
    """isf_attention_backward (rows + cols kernels) vs torch autograd of the same formula in float64: few keys, the
    32400 x 200-shaped case (more queries than keys), the many-keys (split-key forward) case, and -- round 5 -- query counts
    large enough for the chunked key-gradient pass (partial buffers + ordered reduce), up to the real 32400 x 200"""
    from isfusion_amd import fusion_ops as ops
    g = torch.Generator().manual_seed(B * 1000 + Lq + Lk)
    q, k, v = [torch.randn((B * n, 128), generator=g) for n in (Lq, Lk, Lk)]
    gout = torch.randn((B * Lq, 128), generator=g)
    qd, kd, vd = [t.double().requires_grad_() for t in (q, k, v)]
    ref = _torch_mha_core(qd, kd, vd, B, Lq, Lk, 8)
    ref.backward(gout.double())
    qg, kg, vg = [t.to(dev).requires_grad_() for t in (q, k, v)]
    out = ops.AttentionFunction.apply(qg, kg, vg, B, Lq, Lk, 128, 8)
    assert (out.detach().cpu().double() - ref.detach()).abs().max().item() < 1e-4
    out.backward(gout.to(dev))
    for got, want, name in ((qg, qd, "dq"), (kg, kd, "dk"), (vg, vd, "dv")):
        err = (got.grad.cpu().double() - want.grad).abs().max().item()
        assert err < 2e-4 * max(1.0, want.grad.abs().max().item()), (name, err)


@pytest.mark.parametrize("S,d,shift", [(12, 128, 0), (12, 128, 1), (16, 128, 1), (9, 256, 1), (12, 256, 0)])
def test_window_attention_backward_matches_torch_autograd(dev, S, d, shift):
    """isf_window_attention_backward vs torch autograd over the explicit window partition (partial edge windows when
    the grid is shifted or not a multiple of 6)"""
    from isfusion_amd import fusion_ops as ops
    B, heads, win = 2, 8, 6
    hd = d // heads
    g = torch.Generator().manual_seed(S * 10 + d + shift)
    qkv = torch.randn((B * S * S, 3 * d), generator=g)
    gout = torch.randn((B * S * S, d), generator=g)
    x = qkv.double().requires_grad_()
    xr = x.view(B, S, S, 3, heads, hd)
    off = win // 2 if shift else 0
    out_ref = torch.zeros((B, S, S, heads, hd), dtype=torch.float64)
    for wy in range((S + off + win - 1) // win):
        for wx in range((S + off + win - 1) // win):
            ys = [y for y in range(wy * win - off, wy * win - off + win) if 0 <= y < S]
            xs = [c for c in range(wx * win - off, wx * win - off + win) if 0 <= c < S]
            if not ys or not xs:
                continue
            blk = xr[:, ys][:, :, xs]                                       # [B, ny, nx, 3, heads, hd]
            t = blk.reshape(B, len(ys) * len(xs), 3, heads, hd)
            qh, kh, vh = [t[:, :, i].transpose(1, 2) for i in range(3)]    # [B, heads, T, hd]
            o = (qh @ kh.transpose(-1, -2) / hd ** 0.5).softmax(-1) @ vh
            o = o.transpose(1, 2).reshape(B, len(ys), len(xs), heads, hd)
            idx_y = torch.tensor(ys).view(-1, 1).expand(len(ys), len(xs))
            idx_x = torch.tensor(xs).view(1, -1).expand(len(ys), len(xs))
            out_ref[:, idx_y, idx_x] = o
    out_ref = out_ref.reshape(B * S * S, d)
    out_ref.backward(gout.double())
    xg = qkv.to(dev).requires_grad_()
    out = ops.WindowAttentionFunction.apply(xg, B, S, d, heads, win, shift)
    assert (out.detach().cpu().double() - out_ref.detach()).abs().max().item() < 1e-4
    out.backward(gout.to(dev))
    err = (xg.grad.cpu().double() - x.grad).abs().max().item()
    assert err < 2e-4 * max(1.0, x.grad.abs().max().item()), err


# ------------------------------------------------------------------------------------------- f16 storage mode
def _f16(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def lexsort4(idx):
    return np.lexsort((idx[:, 3], idx[:, 2], idx[:, 1], idx[:, 0]))


def _oracle_encoder_f16_storage(oracle_mod, plan, vf, vc, B):
    """the oracle's SparseEncoder with the data types of the reference's fp16 path (indice_conv_half, src/all.cc:35-37):
    f16 features between the layers, f16 weights (scaled by a power of two first, as the packed filters are: exact),
    fp32 accumulation, BN / residual / ReLU in fp32, f16 result"""
    feats, idx, shape = _f16(vf), vc, list(plan["sparse_shape"])
    outs, cache = [], {}
    first = feats
    for L in plan["layers"]:
        subm = L["kind"] == "subm"
        key = ("subm", tuple(shape), tuple(L["ksize"]))
        if subm and key in cache:
            out_idx, pairs, num = cache[key]
        else:
            out_idx, pairs, num = oracle_mod.get_indice_pairs(idx, B, shape, L["ksize"], L["stride"], L["padding"], subm=subm)
            if subm:
                cache[key] = (out_idx, pairs, num)
        w = np.asarray(L["weight"], np.float32)
        amax = np.abs(w).max()
        sw = 2.0 ** (13 - int(np.frexp(amax)[1])) if amax > 0 else 1.0      # pack_filters16_kernel: max|w| 2^sw in [2^12, 2^13)
        y = oracle_mod.indice_conv(feats, _f16(w * sw) / sw, pairs, num, out_idx.shape[0])
        res = None
        if L.get("residual_from") is not None:
            r = L["residual_from"]
            res = outs[r] if r >= 0 else first
        feats = _f16(oracle_mod.bn_act(y, L["scale"], L["shift"], res, L["relu"]))
        if not subm:
            shape = oracle_mod.conv_out_shape(shape, L["ksize"], L["stride"], L["padding"])
            cache = {}
        idx = out_idx
        outs.append(feats)
    return oracle_mod.dense_bev(feats, idx, B, shape)


def test_f16_storage_mode_matches_the_f16_oracle_and_is_off_by_default(dev, oracle_mod):
    """precision 2 (isf_encoder_options, per call; BASELINE configs[4] dtype): activations travel between the layers as
    f16 rows (2 bytes per element), f16 operands, fp32 accumulation -- the reference's indice_conv_half.  Checked
    against the oracle run with exactly those data types (the only differences left are summation order and the
    occasional double rounding), and loosely against the fp32 oracle; the next call is back on the default."""
    import isfusion_amd as m
    from isfusion_amd import synthetic
    from isfusion_amd.norm import fold_bn
    B = 2
    lb = m.LidarBranch().randomize_weights_(0).randomize_bn_(1).eval()
    pl = [synthetic.lidar_sweeps(300 + i, 4000) for i in range(B)]
    coors = np.concatenate([np.concatenate([np.full((p.shape[0], 1), b, np.int32),
                                            oracle_mod.dynamic_voxelize(p, VS, RG)], 1) for b, p in enumerate(pl)])
    vfe = lb.pts_voxel_encoder
    bn1 = [t.numpy() for t in fold_bn(vfe.vfe_layers[0].norm)]
    bn2 = [t.numpy() for t in fold_bn(vfe.vfe_layers[1].norm)]
    ovf, ovc, _ = oracle_mod.dynamic_vfe(np.concatenate(pl), coors, VS, RG,
                                         vfe.vfe_layers[0].linear.weight.detach().numpy(), bn1,
                                         vfe.vfe_layers[1].linear.weight.detach().numpy(), bn2)
    plan = lb.pts_middle_encoder.plan_to_numpy()
    obev, _ = oracle_mod.sparse_encoder_forward(plan, ovf, ovc, B)
    obev16 = _oracle_encoder_f16_storage(oracle_mod, plan, ovf, ovc, B)
    lb = lb.to(dev)
    pts = [_T(p, dev) for p in pl]
    half = lb(pts, precision=2).cpu().numpy()
    full = lb(pts).cpu().numpy()                             # the next call is back on the default: no global state
    scale = np.abs(obev).max()
    assert np.abs(full - obev).max() < 1e-3                  # default path untouched
    err16 = np.abs(half - obev16).max()
    assert err16 < 4e-3 * scale, (err16, scale)              # same data types: a few f16 ulps of the largest features
    err32 = np.abs(half - obev).max()
    assert 10 * 1e-3 < err32 + 1e-2 and err32 < 3e-2 * scale and err32 > 10 * np.abs(full - obev).max()   # not fp32-class
    assert ((half != 0) != (obev16 != 0)).mean() < 1e-3      # ReLU outputs next to zero may flip


@pytest.mark.parametrize("cin,cout", [(64, 32), (32, 32), (64, 64), (128, 128), (256, 256)])
def test_f16_storage_conv_op(dev, oracle_mod, cin, cout):
    """isf_sparse_conv_forward_f16x3 mode CONV_MODE_F16_STORAGE: f16 rows in (features, residual), f16 rows out"""
    from isfusion_amd import _lib, spconv as sp
    rng = np.random.default_rng(cin + 3 * cout)
    B, shape = 2, [9, 24, 20]
    n = 1500
    lin = np.sort(rng.choice(B * int(np.prod(shape)), n, replace=False))
    D, H, W = shape
    idx = np.stack([lin // (D * H * W), (lin // (H * W)) % D, (lin // W) % H, lin % W], 1).astype(np.int32)
    feats = _f16(rng.normal(0, 1, (n, cin)))
    w = rng.normal(0, (1.0 / (6 * cin)) ** 0.5, (3, 3, 3, cin, cout)).astype(np.float32)
    sw = 2.0 ** (13 - int(np.frexp(np.abs(w).max())[1]))
    scale = (rng.random(cout, dtype=np.float32) + 0.5)
    shift = rng.normal(0, 0.2, cout).astype(np.float32)
    for subm, st, pd in ((True, [1, 1, 1], [1, 1, 1]), (False, [2, 2, 2], [1, 1, 1])):
        rb = sp.build_rulebook(T(idx, dev), B, shape, [3, 3, 3], st, pd, subm)
        oidx, pairs, num = oracle_mod.get_indice_pairs(idx, B, shape, [3, 3, 3], st, pd, subm=subm)
        res = _f16(rng.normal(0, 1, (rb.num_out, cout)))
        out_idx = rb.out_indices.cpu().numpy()
        o1, o2 = lexsort4(out_idx), lexsort4(oidx)
        raw = oracle_mod.indice_conv(feats, _f16(w * sw) / sw, pairs, num, len(oidx))[o2]
        want = _f16(oracle_mod.bn_act(raw, scale, shift, res[o1], relu=True))
        got = sp.sparse_conv_forward_f16x3(T(feats, dev), sp.pack_filters_f16x3(T(w, dev)), 27, cin, cout, rb,
                                           T(scale, dev), T(shift, dev), T(res, dev), relu=True,
                                           mode=_lib.CONV_MODE_F16_STORAGE).cpu().numpy()
        # one f16 ulp of the result (fp32 sums agree to 1e-6; rounding to f16 may land on either neighbour)
        assert np.abs(got[o1] - want).max() <= 2.0 ** -10 * max(1.0, np.abs(want).max()), (cin, cout, subm)


# ------------------------------------------------------------------------------------------- neck on the linear kernel
def test_neck_on_linear_kernel_matches_stock_modules(dev):
    """SECONDFPN(dense_conv="hip"): 1x1 conv and 2x2 transposed conv as fused f16x3 GEMMs vs MIOpen"""
    from isfusion_amd.fusion_modules import SECONDFPN, seeded_state_dict
    neck = SECONDFPN().eval()
    neck.load_state_dict(seeded_state_dict(neck, 250))
    neck = neck.to(dev)
    g = torch.Generator().manual_seed(1)
    x = [torch.randn((2, 128, 180, 180), generator=g).to(dev), torch.randn((2, 256, 90, 90), generator=g).to(dev)]
    assert neck.dense_conv == "hip"    # the default
    with torch.no_grad():
        got = neck(x)[0]
        neck.dense_conv = "stock"
        want = neck(x)[0]
    assert got.shape == want.shape == (2, 512, 180, 180)
    assert (got - want).abs().max().item() < 1e-4 * max(1.0, want.abs().max().item())


# ------------------------------------------------------------------------------------------- encoder wiring golden
@pytest.mark.parametrize("name", ["isfusion", "conv_module"])
def test_sparse_encoder_matches_reference_module_tree_golden(dev, golden, name):
    """HIP SparseEncoder (fused engine and module-by-module path) vs the reference's own module tree output"""
    import isfusion_amd as m
    from encoder_common import ENCODER_CASES, encoder_input
    g = golden("encoder_ref.npz")
    case = ENCODER_CASES[name]
    lb = m.LidarBranch(pts_middle_encoder=dict(case["cfg"]))
    lb = lb.randomize_weights_(case["seed"]).randomize_bn_(case["seed"] + 1).eval().to(dev)
    feats, coors, B = encoder_input(case)
    enc = lb.pts_middle_encoder
    out = enc.forward_fused(_T(feats, dev), _T(coors, dev), B)
    assert list(out.shape) == g[name + ".shape"].tolist()
    assert np.abs(out.cpu().numpy().reshape(-1)[g[name + ".idx"]] - g[name + ".val"]).max() < 1e-3
    with torch.no_grad():
        out2, enc_feats = enc.forward_modules(_T(feats, dev), _T(coors, dev), B)
    assert np.abs(out2.cpu().numpy().reshape(-1)[g[name + ".idx"]] - g[name + ".val"]).max() < 1e-3
    assert [int(t.features.shape[0]) for t in enc_feats] == g[name + ".stage_voxels"].tolist()
    # the drop-in forward() on the fused path: same BEV tensor, and encode_features is the reference's per-stage list,
    # computed only when somebody reads it (mmdet3d/models/middle_encoders/sparse_encoder.py:131-138)
    with torch.no_grad():
        out3, lazy, kw = enc(_T(feats, dev), _T(coors, dev), B)
    assert torch.equal(out3, out) and kw == {} and "not computed" in repr(lazy)
    assert [int(t.features.shape[0]) for t in lazy] == g[name + ".stage_voxels"].tolist() and len(lazy) == len(enc_feats)
    assert torch.equal(lazy[-1].features, enc_feats[-1].features)


@pytest.mark.parametrize("name,seed,B,P", [("b2", 41, 2, 3000), ("b1", 43, 1, 5000)])
def test_dynamic_vfe_matches_reference_module_golden(dev, golden, oracle_mod, name, seed, B, P):
    """HIP DynamicVFE (fused C call) vs the reference's DynamicVFE module output"""
    import isfusion_amd as m
    from isfusion_amd import synthetic
    g = golden("dynvfe_ref.npz")
    pl = []
    for i in range(B):
        p = synthetic.lidar_sweeps(seed + i, P)
        pl.append(p[(oracle_mod.dynamic_voxelize(p, VS, RG) >= 0).all(1)])
    coors = np.concatenate([np.concatenate([np.full((p.shape[0], 1), b, np.int32),
                                            oracle_mod.dynamic_voxelize(p, VS, RG)], 1) for b, p in enumerate(pl)])
    vfe = m.LidarBranch().randomize_weights_(seed).randomize_bn_(seed + 1).eval().pts_voxel_encoder.to(dev)
    vf, vc = vfe(_T(np.concatenate(pl), dev), _T(coors, dev))
    assert np.array_equal(vc.cpu().numpy(), g[name + ".voxel_coors"])
    assert np.abs(vf.cpu().numpy()[::4] - g[name + ".voxel_feats_every4"]).max() < 1e-4


# ------------------------------------------------------------------------------------------- detector-level golden
def test_extract_pts_feat_and_neck_match_reference_detector_golden(dev, golden, oracle_mod):
    """ISFusionPtsPath.extract_pts_feat + pts_neck (raw sweeps + camera features -> [B,512,180,180]) vs the
    REFERENCE's ISFusionDetector.extract_pts_feat executed on the CPU (detector_ref.npz); 1e-3 (north_star)"""
    from detector_common import build_path, detector_inputs
    g = golden("detector_ref.npz")
    net = build_path().to(dev)
    pts, inp, kw, metas = detector_inputs()
    img_feats = tuple(torch.from_numpy(a).to(dev) for a in inp["img_feats"])
    feats = net.extract_pts_feat([_T(p, dev) for p in pts], img_feats, metas, **kw)
    with torch.no_grad():
        out = net.pts_neck(feats)[0]
    assert list(out.shape) == g["shape"].tolist()
    flat = out.cpu().numpy().reshape(-1)
    assert np.abs(flat[g["idx"]] - g["val"]).max() < 1e-3
