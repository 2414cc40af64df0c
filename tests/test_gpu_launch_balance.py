"""Equal-work XCD parts of the sparse-conv launches of several rounds (isf_sparse_conv_part_table /
isf_sparse_conv_forward_parts): the launch on its part table computes every row with the same tile as
the plain launch, so the split output rows must be equal bit for bit; the table read back from the device must satisfy the
invariants tests/test_part_plan.py checks on the host arithmetic.  Small launches are planned as if they ran in several
rounds (the builder's flag), so that a few hundred rows exercise the planner."""
import numpy as np
import pytest
import torch

from isfusion_amd import _lib
from test_part_plan import check_invariants

pytestmark = pytest.mark.gpu

SIZES = (1, 127, 8 * 128, 8 * 128 + 1, 11 * 128 + 37, 40 * 128)
DENSITIES = ("uniform", "first eighth", "last tile", "centre only")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _subm_cells(rng, n, density):
    """n active cells (b, z, y, x) in (z, y, x) order of a 1 x 64 x 96 x 96 grid.  Lone cells sit on the even lattice (no two
    of them are neighbours); a dense cluster is a run of consecutive cells of one z plane."""
    H = W = 96

    def lone(count, z0):      # even lattice from plane z0 (even) up
        per = (H // 2) * (W // 2)
        i = np.arange(count)
        return np.stack([np.zeros(count, int), z0 + 2 * (i // per), 2 * ((i % per) // (W // 2)), 2 * (i % (W // 2))], 1)

    def cluster(count, z):    # consecutive cells of plane z (and the planes above it)
        i = np.arange(count)
        return np.stack([np.zeros(count, int), z + i // (H * W), (i % (H * W)) // W, i % W], 1)

    if density == "uniform":
        lin = np.sort(rng.choice(16 * H * W, n, replace=False))
        idx = np.stack([np.zeros(n, int), lin // (H * W), (lin // W) % H, lin % W], 1)
    elif density == "first eighth":
        c = max(1, n // 8)
        idx = np.concatenate([cluster(c, 0), lone(n - c, 4)])
    elif density == "last tile":
        c = min(n, 100)
        idx = np.concatenate([lone(n - c, 0), cluster(c, 60)])
    else:
        idx = lone(n, 0)
    assert len(idx) == n and idx[:, 1].max() < 64
    return idx.astype(np.int32)


def _synthetic_table(rng, n_out, n_in, K, density, stride):
    """a dense neighbour table [K, stride] with the given pattern of present taps (any row of the input may be a neighbour)"""
    nbr = np.full((K, stride), -1, np.int32)
    rows = np.arange(n_out)
    nbr[K // 2, rows] = rng.integers(0, n_in, n_out)
    if density == "uniform":
        sel = rng.random((K, n_out)) < 0.3
    elif density == "first eighth":
        sel = np.zeros((K, n_out), bool)
        sel[:, :max(1, n_out // 8)] = True
    elif density == "last tile":
        sel = np.zeros((K, n_out), bool)
        sel[:, max(0, n_out - 100):] = rng.random((K, min(n_out, 100))) < 0.8
    else:
        sel = np.zeros((K, n_out), bool)
    vals = rng.integers(0, n_in, (K, n_out)).astype(np.int32)
    nbr[:, :n_out] = np.where(sel, vals, nbr[:, :n_out])
    return nbr


def _table_record(pt):
    t = pt.table.cpu().numpy()
    p, cap = pt.parts, pt.cap
    w = pt.weights.cpu().numpy().tolist()
    rec = dict(cap=cap, first=t[:p + 1].tolist(), bound=t[p + 1:p + 4].tolist(),
               slots=[t[p + 4 + k * cap:p + 4 + (k + 1) * cap].tolist() for k in range(p)])
    W, total, cuts = np.cumsum(w), int(np.sum(w)), [0]
    for k in range(1, p):
        reach = np.nonzero(W * p >= k * total)[0]
        cuts.append(int(reach[0]) + 1 if len(reach) else len(w))
    rec["cuts"] = cuts + [len(w)]
    return w, rec


def _plain(sp, kind, xs, p16, K, cin, cout, rb, scale, shift, rs, relu, mode):
    """the plain entry point of the same launch -> the raw output rows"""
    lib = _lib.load()
    ys = torch.empty(rb.num_out * cout * (2 if mode == _lib.CONV_MODE_F16_STORAGE else 4), dtype=torch.uint8, device=xs.device)
    if kind == "lines":
        lines, mask, _flag = sp.rulebook_lines(rb, 3)
        _lib.check(lib.isf_sparse_conv_forward_dma_lines(_lib.ptr(xs), rb.num_in, cin, _lib.ptr(p16), K, 3, cout, _lib.ptr(lines),
                                                         _lib.ptr(mask), rb.stride, rb.num_out, _lib.ptr(scale), _lib.ptr(shift),
                                                         _lib.ptr(rs), int(relu), _lib.ptr(ys), mode, _lib.stream()))
    elif kind == "dma":
        _lib.check(lib.isf_sparse_conv_forward_dma(_lib.ptr(xs), rb.num_in, cin, _lib.ptr(p16), K, cout, _lib.ptr(rb.nbr), rb.stride,
                                                   rb.num_out, _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(rs), int(relu),
                                                   _lib.ptr(ys), mode, None, _lib.stream()))
    else:
        _lib.check(lib.isf_sparse_conv_forward_f16x3(_lib.ptr(xs), rb.num_in, cin, _lib.ptr(p16), K, cout, _lib.ptr(rb.nbr), rb.stride,
                                                     rb.num_out, _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(rs), int(relu),
                                                     _lib.ptr(ys), mode, _lib.stream()))
    return ys


def _parts(sp, kind, xs, p16, K, cin, cout, rb, scale, shift, rs, relu, mode, pt):
    lib = _lib.load()
    ys = torch.empty(rb.num_out * cout * (2 if mode == _lib.CONV_MODE_F16_STORAGE else 4), dtype=torch.uint8, device=xs.device)
    table, mask, nx = rb.nbr, None, 0
    if kind == "lines":
        table, mask, _flag = sp.rulebook_lines(rb, 3)
        nx = 3
    _lib.check(lib.isf_sparse_conv_forward_parts(_lib.ptr(xs), rb.num_in, cin, _lib.ptr(p16), K, nx, cout, _lib.ptr(table),
                                                 _lib.ptr(mask), rb.stride, rb.num_out, _lib.ptr(scale), _lib.ptr(shift),
                                                 _lib.ptr(rs), int(relu), _lib.ptr(ys),
                                                 mode | (0 if kind == "tile" else _lib.CONV_MODE_DMA_PLAN), _lib.ptr(pt.table),
                                                 _lib.stream()), "isf_sparse_conv_forward_parts")
    return ys


# (kernel, c_in, c_out, residual, mode): 32 -> 32 and 64 -> 64 on line tables with and without a residual, 32 -> 64 on a dense
# table with n_in != n_out, 64 -> 128 on the tile kernel, one case in f16 storage
KERNELS = [("lines", 32, 32, False, 0), ("lines", 32, 32, True, 0), ("lines", 64, 64, False, 0), ("lines", 64, 64, True, 0),
           ("dma", 32, 64, False, 0), ("tile", 64, 128, True, 0), ("lines", 64, 64, True, _lib.CONV_MODE_F16_STORAGE)]


@pytest.mark.parametrize("kind,cin,cout,with_res,mode", KERNELS)
def test_balanced_launch_reproduces_the_plain_launch_bits(dev, kind, cin, cout, with_res, mode):
    from isfusion_amd import spconv as sp
    lib = _lib.load()
    rng = np.random.default_rng(cin * 1000 + cout + int(with_res))
    K = 27
    w = T(rng.normal(0, (1.0 / (9 * cin)) ** 0.5, (3, 3, 3, cin, cout)).astype(np.float32), dev)
    p16 = sp.pack_filters_f16x3(w)
    scale, shift = T(rng.random(cout, dtype=np.float32) + 0.5, dev), T(rng.normal(0, 0.2, cout).astype(np.float32), dev)
    f16io = mode == _lib.CONV_MODE_F16_STORAGE
    conv = (lambda a: sp.to_half(a)) if f16io else (lambda a: sp.to_split(a))
    for n in SIZES:
        for density in DENSITIES:
            if kind == "lines":
                idx = _subm_cells(rng, n, density)
                rb = sp.build_rulebook(T(idx, dev), 1, [64, 96, 96], [3, 3, 3], [1, 1, 1], [1, 1, 1], True)
                n_in = n
            else:
                n_in = 2 * n + 5                                    # a strided conv's table: other rows in than out
                stride = lib.isf_nbr_stride(n)
                rb = sp.Rulebook(T(_synthetic_table(rng, n, n_in, K, density, stride), dev), stride, n_in, n, None, None)
            xs = conv(T(rng.normal(0, 1, (n_in, cin)).astype(np.float32), dev))
            rs = conv(T(rng.normal(0, 1, (n, cout)).astype(np.float32), dev)) if with_res else None
            want = _plain(sp, kind, xs, p16, K, cin, cout, rb, scale, shift, rs, True, mode)
            for raster in (False, True):
                pt = sp.part_table(rb, cin, cout, mode, dma=kind != "tile", lines=kind == "lines", several_rounds=True,
                                   raster=raster)
                assert pt is not None and pt.parts == 8
                weights, rec = _table_record(pt)
                check_invariants(weights, pt.parts, rec, raster)
                assert pt.tiles == len(weights) and pt.tiles % 8 == 0 and min(weights) >= 0 and weights[0] > 0
                got = _parts(sp, kind, xs, p16, K, cin, cout, rb, scale, shift, rs, True, mode, pt)
                assert torch.equal(got, want), (kind, cin, cout, n, density, raster)
            assert want.any().item()
    # a launch of one round gets no table unless it is asked for
    assert sp.part_table(rb, cin, cout, mode, dma=kind != "tile", lines=kind == "lines") is None


def test_encoder_default_reproduces_equal_row_raster_bits(dev):
    """isf_sparse_encoder_forward on 250 k voxels, half of them packed into one z slab: the 32 -> 32 launches of the input
    level run in several rounds, on part tables by default; diagnostic 96 (uniform tiles | launch order) keeps the equal-row
    parts in tile order -- the same bits, and so must 32 and 64 alone give"""
    from isfusion_amd.sparse_encoder import SparseEncoder
    rng = np.random.default_rng(5)
    D, H, W = 9, 448, 448
    slab = rng.choice(H * W, 125000, replace=False) + 4 * H * W
    rest = rng.choice(D * H * W, 140000, replace=False)
    lin = np.unique(np.concatenate([slab, rest[(rest // (H * W)) != 4][:125000]]))
    coors = np.stack([np.zeros(len(lin), int), lin // (H * W), (lin // W) % H, lin % W], 1).astype(np.int32)
    assert 240000 <= len(lin) <= 250000
    torch.manual_seed(0)
    enc = SparseEncoder(32, [D, H, W], base_channels=32, output_channels=32, encoder_channels=((32,),),
                        encoder_paddings=((1,),)).eval()
    from isfusion_amd.spconv import SparseConvolution
    g = torch.Generator().manual_seed(1)
    for mod in enc.modules():       # weights sized for the sparse fan-in (LidarBranch.randomize_weights_): the default init
        if isinstance(mod, SparseConvolution):     # shrinks activations to 1e-4 over three layers
            with torch.no_grad():
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (1.0 / (9.0 * mod.in_channels)) ** 0.5)
    enc = enc.to(dev)
    feats = T(rng.normal(0, 1, (len(lin), 32)).astype(np.float32), dev)
    want = enc.forward_fused(feats, T(coors, dev), 1, conv_diag=_lib.ENC_DIAG_UNIFORM_TILES | _lib.ENC_DIAG_LAUNCH_ORDER)
    assert torch.isfinite(want).all() and want.abs().max().item() > 0.05
    assert torch.equal(enc.forward_fused(feats, T(coors, dev), 1), want)
    assert torch.equal(enc.forward_fused(feats, T(coors, dev), 1, conv_diag=_lib.ENC_DIAG_UNIFORM_TILES), want)
    assert torch.equal(enc.forward_fused(feats, T(coors, dev), 1, conv_diag=_lib.ENC_DIAG_LAUNCH_ORDER), want)
