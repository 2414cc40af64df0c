"""The LiDAR branch's training step restated in plain torch, dtype-generic: DynamicVFE (cluster centre, voxel centre, max
pooling) and the SparseEncoder layer list, both with batch-statistic BatchNorm.  The parameters are leaves in the dtype
asked for, so the same code is the float64 reference and the float32 stock-torch baseline of
tests/test_gpu_lidar_train.py; tests/test_lidar_train.py pins it to the CPU oracle first.

No isfusion_amd kernel and no oracle arithmetic in here: oracle.get_indice_pairs / conv_out_shape (and, in the input
builders, oracle.dynamic_voxelize) supply integer geometry only."""
import ast
import os

import numpy as np
import torch

import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 1e-3                                     # every BatchNorm of the branch (norm_cfg eps of the shipped config)
MOMENTUM = 0.01
# a 48 x 48 x 41 window as the whole grid: D = 41 keeps the shipped 41 -> 21 -> 11 -> 5 -> 2 depth chain and the [0, 1, 1]
# padding; voxel edges are binary fractions, so cell centres are exact in float32 and float64 alike
SPARSE_SHAPE = [41, 48, 48]
VOXEL_SIZE = [0.5, 0.5, 0.25]
PC_RANGE = [-12.0, -12.0, -5.0, 12.0, 12.0, 5.25]
# voxels of 2 ... 30 points in sample 0 (a quarter as many in sample 1) and their sizes; the rest of a sample's 600 points sit
# alone in their voxel.  More of them, or more points, and no seed meets the near-tie precondition: the smallest gap between
# the two largest values falls as 1 / (voxels of several points x 64 channels), the float32 error does not
MULTI_VOXELS = 20
MODEL_SEED = 40
# point_clouds seeds picked on the CPU, of 2500 to 16000 tried each.  About one in a thousand clears assert_no_near_ties;
# of those, the ones whose ReLU inputs in the encoder's last two levels (tens of rows: one ReLU that changes side there
# moves a BatchNorm gradient by a tenth) stay clear of zero.  Tie margins: 120 (blobs), 130, 180, where 100 is asked.
# Seeds with a wider tie margin for blobs (1197, 13450) had a ReLU input at zero instead.
POINT_SEEDS = dict(blobs=4921, one_voxel=1343, empty=3321)
MULTI_SIZES = [2, 2, 2, 2, 3, 3, 3, 4, 4, 5, 6, 8, 12, 20, 30]


# ------------------------------------------------------------------------------------------------------------ modules
def branch_config():
    """LidarBranch kwargs: the shipped module tree (tests/golden/isfusion_0075voxel_model.txt) on the small grid"""
    with open(os.path.join(HERE, "golden", "isfusion_0075voxel_model.txt")) as f:
        model = ast.literal_eval(f.read())
    ve, me = dict(model["pts_voxel_encoder"]), dict(model["pts_middle_encoder"])
    ve.update(voxel_size=VOXEL_SIZE, point_cloud_range=PC_RANGE)
    me.update(sparse_shape=SPARSE_SHAPE)
    return dict(voxel_size=VOXEL_SIZE, point_cloud_range=PC_RANGE, pts_voxel_encoder=ve, pts_middle_encoder=me)


def make_branch(seed):
    """a seeded LidarBranch on the CPU: O(1) activations, non-trivial BatchNorm buffers and affine parameters"""
    from isfusion_amd import LidarBranch
    torch.manual_seed(seed)
    return LidarBranch(**branch_config()).randomize_weights_(seed).randomize_bn_(seed + 1)


def encoder_modules(enc):
    """[(conv, bn)] in the order of enc.export_plan()["layers"]"""
    from isfusion_amd.spconv import SparseConvolution
    convs = [m for m in enc.modules() if isinstance(m, SparseConvolution)]
    bns = [m for m in enc.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    plan = enc.export_plan()["layers"]
    assert len(convs) == len(bns) == len(plan) and all(L["conv"] is c for L, c in zip(plan, convs))
    return list(zip(convs, bns))


def _leaf(t, dtype, device):
    return t.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)


def vfe_params(vfe, dtype, device):
    """leaf copies of the DynamicVFE's parameters: [dict(weight [N, K], gamma, beta)] per layer"""
    return [dict(weight=_leaf(l.linear.weight, dtype, device), gamma=_leaf(l.norm.weight, dtype, device),
                 beta=_leaf(l.norm.bias, dtype, device)) for l in vfe.vfe_layers]


def encoder_params(enc, dtype, device):
    """leaf copies of the SparseEncoder's parameters: [dict(weight [kD, kH, kW, Cin, Cout], gamma, beta)] per plan layer"""
    return [dict(weight=_leaf(c.weight, dtype, device), gamma=_leaf(b.weight, dtype, device),
                 beta=_leaf(b.bias, dtype, device)) for c, b in encoder_modules(enc)]


def batch_norm(y, gamma, beta):
    """BatchNorm1d with batch statistics over the rows -> (output, batch mean, biased batch variance)"""
    mean = y.mean(0)
    var = y.var(0, unbiased=False)
    return (y - mean) * torch.rsqrt(var + EPS) * gamma + beta, mean, var


# ---------------------------------------------------------------------------------------------------------------- VFE
def voxel_index(coors4):
    """(b, z, y, x) of every point -> (point -> voxel map [P], voxel coordinates [M, 4] sorted (b, z, y, x), count [M])"""
    c = coors4.long()
    assert int(c.min()) >= 0, "drop the out-of-range points first"
    d = c.max(0).values + 1
    key = ((c[:, 0] * d[1] + c[:, 1]) * d[2] + c[:, 2]) * d[3] + c[:, 3]
    uniq, inv, count = torch.unique(key, return_inverse=True, return_counts=True)     # sorted keys = sorted (b, z, y, x)
    x, rest = uniq % d[3], uniq // d[3]
    y, rest = rest % d[2], rest // d[2]
    return inv, torch.stack([rest // d[1], rest % d[1], y, x], 1), count


def first_argmax(values, inv, count):
    """[M, C] point index of each voxel's per-channel maximum and of its runner-up.  Among points that hold the same value
    the LOWEST index wins: the reference's gradient convention (scatter_points_cuda.cu: the first point whose value equals
    the maximum receives the gradient).  Voxels of one point name that point twice."""
    with torch.no_grad():
        by_value = torch.argsort(values, dim=0, descending=True, stable=True)        # ties keep ascending point order
        by_voxel = torch.argsort(inv[by_value], dim=0, stable=True)
        order = by_value.gather(0, by_voxel)                                           # per channel: voxel runs, best first
        start = torch.cumsum(count, 0) - count
        return order[start], order[start + (count > 1).long()]


def vfe_train(params, points, coors4, fold=None, voxel_size=VOXEL_SIZE, pc_range=PC_RANGE):
    """DynamicVFE._forward_composed restated.  points [P, C] (a leaf, or not), coors4 [P, 4] integer (b, z, y, x), all in
    range; fold: per layer (scale, shift) of an eval-mode BatchNorm instead of batch statistics.
    -> dict(voxel_feats [M, N], voxel_coors [M, 4], inv, count, pre_max / arg / second per layer, stats per layer)"""
    inv, vcoors, count = voxel_index(coors4)
    M = count.numel()
    dt = points.dtype
    xyz = points[:, :3]
    mean = torch.zeros((M, 3), dtype=dt, device=points.device).index_add(0, inv, xyz) / count.to(dt)[:, None]
    centre = torch.stack([coors4[:, 3 - j].to(dt) * voxel_size[j] + (voxel_size[j] / 2 + pc_range[j]) for j in range(3)], 1)
    x = torch.cat([points, xyz - mean[inv], xyz - centre], 1)
    out = dict(voxel_coors=vcoors, inv=inv, count=count, pre_relu=[], pre_max=[], arg=[], second=[], stats=[])
    for i, p in enumerate(params):
        y = x @ p["weight"].t()
        if fold is not None:
            y, mu, var = y * fold[i][0] + fold[i][1], None, None
        else:
            y, mu, var = batch_norm(y, p["gamma"], p["beta"])
        pf = torch.relu(y)
        arg, second = first_argmax(pf.detach(), inv, count)
        vmax = pf.gather(0, arg)
        out["pre_relu"].append(y.detach())
        out["pre_max"].append(pf)
        out["arg"].append(arg)
        out["second"].append(second)
        out["stats"].append((mu, var, pf.shape[0], None))
        x = torch.cat([pf, vmax[inv]], 1)
    out["voxel_feats"] = vmax
    return out


def tie_margin(r64, r32):
    """The near-tie precondition's two figures per VFE layer, from the restatement alone: over every (voxel, channel) with
    at least two points and a positive maximum in the float64 run, (the smallest gap between the two largest values, the
    largest |float32 - float64| difference of those voxels' pre-max values)."""
    res = []
    for pf, pf32, arg, second in zip(r64["pre_max"], r32["pre_max"], r64["arg"], r64["second"]):
        pf = pf.detach()
        top, sec = pf.gather(0, arg), pf.gather(0, second)
        ok = (r64["count"] > 1)[:, None] & (top > 0)
        assert bool(ok.any())
        diff = (pf32.detach().double() - pf).abs()
        res.append((float((top - sec)[ok].min()), float(diff[ok[r64["inv"]]].max())))
    return res


def kink_margin(r64, r32):
    """The ReLU's side of the same precondition, per VFE layer: (the smallest |pre-activation| that carries a gradient, the
    largest |float32 - float64| difference of the layer's pre-activations).  Layer 1 feeds every point's value to layer 2,
    so every element counts; the last layer is read through the per-voxel maximum only, so there the voxel's largest
    pre-activation counts (negative: the whole voxel is zero and stays so)."""
    res, last = [], len(r64["pre_relu"]) - 1
    for layer, (y, y32) in enumerate(zip(r64["pre_relu"], r32["pre_relu"])):
        if layer == last:
            M = r64["count"].numel()
            idx = r64["inv"][:, None].expand_as(y)
            top = torch.full((M, y.shape[1]), -float("inf"), dtype=y.dtype, device=y.device).scatter_reduce(0, idx, y, "amax")
            near = float(top.abs().min())
        else:
            near = float(y.abs().min())
        res.append((near, float((y32.double() - y).abs().max())))
    return res


def assert_no_near_ties(r64, r32):
    """the precondition of the comparisons with the HIP step, on the restatement alone.  Ties of the maximum: 100 x the
    float32 difference, as an argmax over up to 97 candidates is at stake.  The ReLU's kink: a derivative flips only where
    two computations disagree about one value's sign, so 10 x the largest float32 difference (the HIP step sits at about
    2 x the float32 error) -- at 100 x no cloud of 600 points qualifies, 40 000 pre-activations of order 1 being in play."""
    for layer, (gap, diff) in enumerate(tie_margin(r64, r32)):
        print(f"vfe layer {layer}: smallest gap of the two largest values {gap:.3e}, largest f32 - f64 difference {diff:.3e}")
        assert gap >= 100 * diff, (layer, gap, diff)
    for layer, (near, diff) in enumerate(kink_margin(r64, r32)):
        print(f"vfe layer {layer}: pre-activation nearest to the ReLU's kink {near:.3e}, largest f32 - f64 difference {diff:.3e}")
        assert near >= 10 * diff, (layer, near, diff)


def assert_cloud_has_no_near_ties(second):
    """assert_no_near_ties for the point cloud point_clouds(POINT_SEEDS[second], second) and the branch make_branch(MODEL_SEED),
    with both sides of the restatement on the CPU: there the float32 side is the same in every run (on a GPU its
    index_add sums with atomics, and the largest float32 - float64 difference was seen to vary by a quarter between runs),
    so the CPU tests and the GPU tests assert one and the same figures"""
    vfe = make_branch(MODEL_SEED).pts_voxel_encoder
    pl = point_clouds(POINT_SEEDS[second], second)
    pts, c4 = np.concatenate(pl), voxelize(pl)
    keep = torch.from_numpy((c4[:, 1:] >= 0).all(1))
    with torch.no_grad():
        runs = [vfe_train(vfe_params(vfe, dt, "cpu"), torch.from_numpy(pts).to(dt)[keep], torch.from_numpy(c4)[keep])
                for dt in (torch.float64, torch.float32)]
    assert all(torch.equal(a, b) for a, b in zip(runs[0]["arg"], runs[1]["arg"]))
    assert_no_near_ties(*runs)
    return runs


# ------------------------------------------------------------------------------------------------------------ encoder
def encoder_geometry(plan, coors, B, device):
    """per plan layer dict(taps=[(k, input rows, output rows)], out_idx [n, 4] int32, shape): the integer side of the
    encoder, by oracle.get_indice_pairs.  SubM layers of one level share one record."""
    idx = np.ascontiguousarray(coors, np.int32)
    shape = list(plan["sparse_shape"])
    layers, level = [], {}
    for L in plan["layers"]:
        subm = L["kind"] == "subm"
        g = level.get(tuple(L["ksize"])) if subm else None
        if g is None:
            out_idx, pairs, num = oracle.get_indice_pairs(idx, B, shape, L["ksize"], L["stride"], L["padding"], subm=subm)
            taps = [(k, torch.from_numpy(pairs[k, 0, :num[k]].astype(np.int64)).to(device),
                     torch.from_numpy(pairs[k, 1, :num[k]].astype(np.int64)).to(device)) for k in range(len(num)) if num[k]]
            if not subm:
                shape = oracle.conv_out_shape(shape, L["ksize"], L["stride"], L["padding"])
                level = {}
            g = dict(taps=taps, out_idx=out_idx, shape=list(shape))
            if subm:
                level[tuple(L["ksize"])] = g
        layers.append(g)
        idx = g["out_idx"]
    return layers


def conv_rows(x, weight, g):
    """one sparse convolution: out[o] += x[i] @ W[k] over the rulebook's (k, i, o) pairs"""
    W = weight.reshape(-1, weight.shape[-2], weight.shape[-1])
    out = torch.zeros((g["out_idx"].shape[0], W.shape[-1]), dtype=x.dtype, device=x.device)
    for k, rows_in, rows_out in g["taps"]:
        out = out.index_add(0, rows_out, x[rows_in] @ W[k])
    return out


def encoder_train(plan, params, voxel_feats, coors, B, fold=False, geometry=None):
    """SparseEncoder.forward_modules restated over the layer list of SparseEncoder.plan_to_numpy() (kind, ksize, stride,
    padding, relu, residual_from).  fold: the plan's eval-mode (scale, shift) instead of batch statistics.
    -> (map [B, C * D, H, W], [rows of every layer], [(batch mean, biased batch variance, rows, the ReLU's input)],
    geometry)"""
    geometry = geometry or encoder_geometry(plan, coors, B, voxel_feats.device)
    x, rows, stats = voxel_feats, [], []
    for L, p, g in zip(plan["layers"], params, geometry):
        y = conv_rows(x, p["weight"], g)
        if fold:
            like = dict(dtype=y.dtype, device=y.device)
            y, mu, var = y * torch.as_tensor(L["scale"]).to(**like) + torch.as_tensor(L["shift"]).to(**like), None, None
        else:
            y, mu, var = batch_norm(y, p["gamma"], p["beta"])
        n = y.shape[0]
        if L["residual_from"] is not None:
            y = y + (rows[L["residual_from"]] if L["residual_from"] >= 0 else voxel_feats)
        x = torch.relu(y) if L["relu"] else y
        rows.append(x)
        stats.append((mu, var, n, y.detach() if L["relu"] else None))
    idx = torch.from_numpy(geometry[-1]["out_idx"].astype(np.int64)).to(x.device)
    D, H, W = geometry[-1]["shape"]
    dense = torch.zeros((B, D, H, W, x.shape[1]), dtype=x.dtype, device=x.device)
    dense = dense.index_put((idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]), x).permute(0, 4, 1, 2, 3)
    return dense.reshape(B, x.shape[1] * D, H, W), rows, stats, geometry


def branch_train(plan, vparams, eparams, points, coors4, B, geometry=None):
    """LidarBranch.forward_train restated: the in-range points through vfe_train, its voxels through encoder_train.
    points [P, C] all samples' points (a leaf), coors4 [P, 4] integer with -1 rows for out-of-range points
    -> (map, the vfe_train record, encoder rows, encoder statistics, geometry)"""
    keep = (coors4[:, 1:] >= 0).all(1)
    v = vfe_train(vparams, points[keep], coors4[keep])
    dense, rows, stats, geometry = encoder_train(plan, eparams, v["voxel_feats"], v["voxel_coors"].cpu().numpy(), B,
                                                 geometry=geometry)
    return dense, v, rows, stats, geometry


# ------------------------------------------------------------------------------------------------------------- inputs
def voxelize(points_list, voxel_size=VOXEL_SIZE, pc_range=PC_RANGE):
    """oracle.dynamic_voxelize per sample -> int32 [sum P, 4] (b, z, y, x); out-of-range points are (b, -1, -1, -1)"""
    return np.concatenate([np.concatenate([np.full((len(p), 1), b, np.int32),
                                           oracle.dynamic_voxelize(p, voxel_size, pc_range)], 1)
                           for b, p in enumerate(points_list)])


def _sample_points(g, cells, sizes):
    lo = np.array(PC_RANGE[:3])
    vs = np.array(VOXEL_SIZE)
    # (x, y, z, intensity 0 ... 255 as the raw sweeps carry it, time lag 0 ... 0.5 s): the intensity varies inside a voxel as
    # much as across the scene, which keeps the points of one voxel apart in every channel of the first layer
    pts = [np.concatenate([lo + (np.array(c[::-1]) + g.uniform(0.05, 0.95, (n, 3))) * vs, g.uniform(0, 255, (n, 1)),
                           g.uniform(0, 0.5, (n, 1))], 1) for c, n in zip(cells, sizes)]
    pts = np.concatenate(pts).astype(np.float32)
    return pts[g.permutation(len(pts))]


def _blob_cells(g, blobs, n, sigma=(2.0, 3.0, 3.0)):
    """n distinct (z, y, x) cells of the grid in Gaussian blobs, so that neighbours exist at every level"""
    D, H, W = SPARSE_SHAPE
    centres = np.stack([g.integers(4, D - 4, blobs), g.integers(6, H - 6, blobs), g.integers(6, W - 6, blobs)], 1)
    cells = set()
    while len(cells) < n:
        c = np.rint(centres[g.integers(0, blobs)] + g.normal(size=3) * sigma).astype(int)
        if (c >= 0).all() and (c < [D, H, W]).all():
            cells.add(tuple(int(v) for v in c))
    return sorted(cells)


def point_clouds(seed, second="blobs", stray=3):
    """two samples of float32 [P, 5] points (about 600 each) inside the window: voxels of 1 to ~30 points, and three voxels
    longer than a 64-lane wave in sample 0; `stray` points of sample 0 lie outside the range.
    second: "blobs" (a sample like the first), "one_voxel" (a single voxel of 3 points) or "empty" (out-of-range points only:
    the sample owns no voxel, so its slice of the dense map is all zeros)"""
    g = np.random.default_rng(seed)
    out = []
    for b in range(2):
        if b == 1 and second == "one_voxel":
            out.append(_sample_points(g, [(20, 30, 17)], [3]))
            continue
        if b == 1 and second == "empty":
            out.append(np.concatenate([g.uniform(30.0, 40.0, (4, 3)), g.random((4, 2))], 1).astype(np.float32))
            continue
        sizes = list(g.choice(MULTI_SIZES, MULTI_VOXELS // (3 * b + 1))) + ([65, 70, 97] if b == 0 else [])
        sizes += [1] * max(600 - sum(sizes), 100)
        cells = _blob_cells(g, 4, len(sizes))
        cells = [cells[i] for i in g.permutation(len(cells))]
        pts = _sample_points(g, cells, sizes)
        if b == 0 and stray:
            pts[:stray, 2] = 100.0
        out.append(pts)
    return out


def blob_voxels(seed=5, B=2, per_sample=1229, blobs=6):
    """the encoder's own case: 2458 active voxels in six Gaussian blobs per sample -> (features float32 [N, 64], coords
    int32 [N, 4] sorted (b, z, y, x), B)"""
    g = np.random.default_rng(seed)
    coors = np.concatenate([np.concatenate([np.full((per_sample, 1), b), np.array(_blob_cells(g, blobs, per_sample))], 1)
                            for b in range(B)]).astype(np.int32)
    feats = g.normal(size=(len(coors), 64)).astype(np.float32)
    return feats, coors, B


def sort_rows(feats, idx):
    """rows in (b, z, y, x) order: the two sides number a strided layer's output sites differently"""
    idx = idx.long()
    d = idx.max(0).values + 1
    key = ((idx[:, 0] * d[1] + idx[:, 1]) * d[2] + idx[:, 2]) * d[3] + idx[:, 3]
    order = torch.argsort(key)
    return feats[order], idx[order]
