"""Sparse convolutions at every kernel geometry on the GPU, against the float64 dense-conv3d reference and the brute-force
tables of tests/conv_geometry_common.py (case table, value distribution and the per-element comparator are described
there; the bound c(n) S is derived, not measured).  One test function per kernel family, one parameter per geometry: a
failure or a fault names one family at one geometry.  Every test prints the largest err / (c(n) S) it saw."""
import numpy as np
import pytest
import torch

import conv_geometry_common as cg

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rulebook(sp, case, dev):
    g = case.geom
    return sp.build_rulebook(T(case.idx, dev), case.batch, list(case.shape), list(g.ks), list(g.st), list(g.pd), g.subm)


class Worst:
    """largest ratio seen per name; every ratio must be within the bound"""

    def __init__(self):
        self.q = {}

    def add(self, what, ratios):
        for name, v in ratios.items():
            assert v <= 1.0, (*what, name, v)
            self.q[name] = max(self.q.get(name, 0.0), v)

    def report(self, family, group, runs):
        print(f"{family} {group}: {runs} runs, largest err / (c(n) S): " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(self.q.items())))
        assert runs > 0


# ------------------------------------------------------------------------------------------------------------ tables
def _lines_can_express(nbr, tpl):
    """does every line of `tpl` taps name consecutive rows in every output row (what the line-compressed form stores)?"""
    K, m = nbr.shape
    for line in range(K // tpl):
        blk = nbr[line * tpl:(line + 1) * tpl]
        have = blk >= 0
        first = np.where(have.any(0), np.where(have, blk, np.iinfo(np.int32).max).min(0), 0)
        # the present entries, in tap order, must be first, first + 1, ...
        want = first[None, :] + np.cumsum(have, 0) - 1
        if not np.array_equal(blk[have], want[have]):
            return False
    return True


@pytest.mark.parametrize("group", cg.GROUPS)
def test_tables(dev, group):
    """build_rulebook, Rulebook.transposed(), pair_lists, the line-compressed form and the stage tables against brute force"""
    from isfusion_amd import _lib, spconv as sp
    lib = _lib.load()
    for case in cg.cases_of(group):
        g, tb = case.geom, cg.tables(case)
        rb = _rulebook(sp, case, dev)
        m = tb.num_out
        assert rb.num_out == m and rb.num_in == case.n, case.id
        assert list(rb.out_shape) == list(g.out_shape(case.shape)), case.id
        assert rb.stride % 128 == 0 and rb.stride >= lib.isf_nbr_stride(m), case.id
        nbr = rb.nbr.cpu().numpy()
        assert nbr.shape == (g.K, rb.stride)
        assert np.array_equal(rb.out_indices.cpu().numpy().reshape(m, 4), tb.out_idx), case.id
        assert np.array_equal(nbr[:, :m], tb.nbr), case.id
        assert (nbr[:, m:] == -1).all(), case.id
        # the transposed view
        rbt = rb.transposed()
        nbr_t = rbt.nbr.cpu().numpy()
        assert rbt.num_in == m and rbt.num_out == case.n and rbt.stride == lib.isf_nbr_stride(case.n)
        assert np.array_equal(nbr_t[:, :case.n], tb.nbr_t) and (nbr_t[:, case.n:] == -1).all(), case.id
        # per-tap pair lists: output-row order, counts, -1 padding
        pairs, num, cap = sp.pair_lists(rb)
        pairs, num = pairs.cpu().numpy(), num.cpu().numpy()
        assert pairs.shape == (g.K, 2, cap) and np.array_equal(num, tb.counts), case.id
        for k in range(g.K):
            c = int(num[k])
            assert np.array_equal(pairs[k, 0, :c], tb.pairs[k][0]) and np.array_equal(pairs[k, 1, :c], tb.pairs[k][1]), (case.id, k)
            assert cap % 32 == 0 and cap >= c + 32, (case.id, k)
            assert (pairs[k, :, c:c + 32] == -1).all(), (case.id, k)      # what the contract pads: 32 entries past the count
        # line-compressed form: a round trip where the form exists, the flag where it cannot (shuffled rows)
        for tpl in (3, 1):
            if g.K % tpl or g.K // tpl > 9:
                continue
            lines, mask, flag = sp.rulebook_lines(rb, tpl)
            assert lines.shape == (g.K // tpl, rb.stride), (case.id, tpl)
            expressible = _lines_can_express(tb.nbr, tpl)
            if g.has_lines(tpl) and (tpl == 1 or not case.shuffled):
                assert expressible, (case.id, tpl)
            assert (int(flag.item()) == 0) == expressible, (case.id, tpl)
            bits = ((tb.nbr >= 0).astype(np.int64) << np.arange(g.K)[:, None]).sum(0)
            got_bits = mask.cpu().numpy().view(np.uint32)
            assert np.array_equal(got_bits[:m], bits.astype(np.uint32)) and not got_bits[m:].any(), (case.id, tpl)
            if expressible:
                assert np.array_equal(sp.lines_to_nbr(lines, mask, g.K, tpl).cpu().numpy(), nbr), (case.id, tpl)
        # stage tables, as test_stage_tables_reconstruct_the_neighbour_table reads them
        slots, ulist, ucount = (t.cpu().numpy() for t in sp.stage_tables(rb))
        slots = slots.view(np.uint16)
        assert slots.shape == (g.K, rb.stride) and ulist.shape[0] == rb.stride // 64 == ucount.shape[0]
        for u in range(rb.stride // 64):
            blk = nbr[:, u * 64:(u + 1) * 64]
            want = np.unique(blk[blk >= 0])
            assert ucount[u] == want.size and np.array_equal(ulist[u, :want.size], want), (case.id, u)
            sl = slots[:, u * 64:(u + 1) * 64]
            assert np.array_equal(sl == 0xFFFF, blk < 0), (case.id, u)
            assert np.array_equal(ulist[u][sl[blk >= 0].astype(np.int64)], blk[blk >= 0]), (case.id, u)


# ------------------------------------------------------------------------------------------------------------ forward
def _f16x3(sp, x, p16, K, ci, co, rb, case):
    return [("plain", sp.sparse_conv_forward_f16x3(x, p16, K, ci, co, rb))]


def _tile(sp, x, p16, K, ci, co, rb, case):
    runs = _f16x3(sp, x, p16, K, ci, co, rb, case)
    order = sp.tile_order(rb, ci, co)
    if order is not None:
        runs.append(("ordered", sp.sparse_conv_forward_f16x3(x, p16, K, ci, co, rb, order=order)))
    return runs


def _dma(sp, x, p16, K, ci, co, rb, case):
    runs = [("launch order", sp.sparse_conv_forward_dma(x, p16, K, ci, co, rb))]
    order = sp.tile_order(rb, ci, co, dma=True)
    if order is not None:
        runs.append(("ordered", sp.sparse_conv_forward_dma(x, p16, K, ci, co, rb, order=order)))
    return runs


def _lines(tpl):
    def run(sp, x, p16, K, ci, co, rb, case):
        assert int(sp.rulebook_lines(rb, tpl)[2].item()) == 0, (case.id, tpl)
        return [(f"{tpl} per line", sp.sparse_conv_forward_dma_lines(x, p16, K, ci, co, rb, taps_per_line=tpl))]
    return run


def _staged(sp, x, p16, K, ci, co, rb, case):
    return [(f"{rows} LDS rows", sp.sparse_conv_forward_staged(x, p16, K, ci, co, rb, stage_rows=rows)) for rows in (512, 32)]


def _cu(sp, x, p16, K, ci, co, rb, case):
    return [("variant 0", sp.sparse_conv_forward_cu(x, p16, K, ci, co, rb))]


def _best(sp, x, p16, K, ci, co, rb, case):
    return [("choice", sp.sparse_conv_forward_best(x, p16, K, ci, co, rb))]


def _fp32(sp, x, p16, K, ci, co, rb, case):
    return [("packed", sp.sparse_conv_forward(x, p16, K, ci, co, rb))]


SPLIT_FAMILIES = {"tile": _tile, "dma": _dma, "dma_lines3": _lines(3), "dma_lines1": _lines(1), "staged": _staged, "cu": _cu,
                  "best": _best}


def _forward_family(dev, family, group):
    """every case of the group on every channel shape the family takes: against float64, and (f16x3 class) bit-identical to
    the plain tile-kernel launch on the same rulebook"""
    from isfusion_amd import spconv as sp
    split = family in SPLIT_FAMILIES
    run = SPLIT_FAMILIES[family] if split else _fp32
    worst, runs = Worst(), 0
    for case in cg.cases_of(group):
        shapes = cg.family_shapes(family, case)
        if not shapes:
            continue
        rb = _rulebook(sp, case, dev)
        assert rb.num_out == cg.tables(case).num_out, case.id
        for ci, co in shapes:
            r = cg.reference(case, ci, co)
            x, w = T(r.x, dev), T(r.w, dev)
            packed = sp.pack_filters_f16x3(w) if split else sp.pack_filters(w)
            base = sp.sparse_conv_forward_f16x3(x, packed, case.geom.K, ci, co, rb) if split else None
            for what, got in run(sp, x, packed, case.geom.K, ci, co, rb, case):
                assert got.shape == (rb.num_out, co)
                worst.add((case.id, ci, co, what), cg.ratios(case, r, out=got.cpu().numpy()))
                if split:
                    assert torch.equal(got, base), (case.id, ci, co, what, (got - base).abs().max().item())
                runs += 1
    if runs == 0:
        assert not any(cg.family_shapes(family, c) for c in cg.cases_of(group))
        print(f"{family} {group}: outside what the family takes")
        return
    worst.report(family, group, runs)


@pytest.mark.parametrize("group", cg.GROUPS)
def test_forward_fp32_mfma(dev, group):
    _forward_family(dev, "fp32_mfma", group)


@pytest.mark.parametrize("group", cg.GROUPS)
def test_forward_generic(dev, group):
    _forward_family(dev, "generic", group)


@pytest.mark.parametrize("group", cg.GROUPS)
def test_forward_tile_kernel(dev, group):
    _forward_family(dev, "tile", group)


@pytest.mark.parametrize("group", cg.GROUPS)
def test_forward_lds_dma(dev, group):
    _forward_family(dev, "dma", group)


@pytest.mark.parametrize("group", [g for g in cg.GROUPS if any(cg.family_shapes("dma_lines3", c) for c in cg.cases_of(g))])
def test_forward_lds_dma_on_lines_of_three(dev, group):
    _forward_family(dev, "dma_lines3", group)


@pytest.mark.parametrize("group", [g for g in cg.GROUPS if any(cg.family_shapes("dma_lines1", c) for c in cg.cases_of(g))])
def test_forward_lds_dma_on_lines_of_one(dev, group):
    _forward_family(dev, "dma_lines1", group)


@pytest.mark.parametrize("group", cg.GROUPS)
def test_forward_staged(dev, group):
    _forward_family(dev, "staged", group)


@pytest.mark.parametrize("group", [g for g in cg.GROUPS if any(cg.family_shapes("cu", c) for c in cg.cases_of(g))])
def test_forward_cu_kernel(dev, group):
    _forward_family(dev, "cu", group)


@pytest.mark.parametrize("group", cg.GROUPS)
def test_forward_kernel_choice(dev, group):
    _forward_family(dev, "best", group)


# ------------------------------------------------------------------------------------------------------------ backward
def _backward(dev, group, shapes):
    """SparseConvFunction: output, dX and dW against float64 in both row orders; a second backward gives the same bits.
    (Weights of magnitude [1/2, 1] at 27 taps x 32 channels make |dX| exceed 64 max |g|: the case that needs the dX filters'
    headroom, spconv.pack_filters_dx -- without it the split rows of dX overflow to NaN.)"""
    from isfusion_amd import spconv as sp
    worst, runs = Worst(), 0
    for case in cg.cases_of(group):
        rb = None
        for ci, co in shapes:
            if not cg.n_ok(case.geom.K, ci, co, backward=True):
                continue
            rb = rb or _rulebook(sp, case, dev)
            r = cg.reference(case, ci, co)
            x, w, g = T(r.x, dev).requires_grad_(True), T(r.w, dev).requires_grad_(True), T(r.g, dev)
            out = sp.SparseConvFunction.apply(x, w, rb)
            assert out.shape == (rb.num_out, co)
            dx, dw = torch.autograd.grad(out, (x, w), g, retain_graph=True)
            dx2, dw2 = torch.autograd.grad(out, (x, w), g)
            assert torch.equal(dx, dx2) and torch.equal(dw, dw2), (case.id, ci, co)
            assert dx.shape == x.shape and dw.shape == w.shape
            worst.add((case.id, ci, co), cg.ratios(case, r, out.detach().cpu().numpy(), dx.cpu().numpy(), dw.cpu().numpy()))
            runs += 1
    if runs == 0:
        assert not any(cg.n_ok(c.geom.K, ci, co, backward=True) for c in cg.cases_of(group) for ci, co in shapes)
        print(f"backward {shapes} {group}: outside the comparator's range")
        return
    worst.report(f"backward {shapes}", group, runs)


@pytest.mark.parametrize("group", cg.GROUPS)
def test_backward_split_precision(dev, group):
    _backward(dev, group, cg.BACKWARD_SPLIT)


@pytest.mark.parametrize("group", cg.GROUPS)
def test_backward_fp32_fallbacks(dev, group):
    _backward(dev, group, cg.BACKWARD_FP32)


# ------------------------------------------------------------------------------------------------------------ modules
def _module(sp, case, ci, co, r, bias, dev):
    g = case.geom
    cls = sp.SubMConv3d if g.subm else sp.SparseConv3d
    kw = {} if g.subm else dict(stride=list(g.st), padding=list(g.pd))
    m = cls(ci, co, list(g.ks), bias=True, **kw).to(dev)
    with torch.no_grad():
        m.weight.copy_(T(r.w, dev))
        m.bias.copy_(T(bias, dev))
    return m


def _with_bias(case, r, bias):
    """(reference, S, n) of conv + bias: one more term per element"""
    return r.out + bias.astype(np.float64), r.s_out + np.abs(bias).astype(np.float64), case.geom.K * r.x.shape[1] + 1


@pytest.mark.parametrize("group", cg.GROUPS)
def test_modules_with_bias_on_shuffled_rows(dev, group):
    """SparseConv3d / SubMConv3d with bias, eval and training mode: output, active set, dX, dW, dbias"""
    from isfusion_amd import spconv as sp
    worst, runs = Worst(), 0
    for case in cg.cases_of(group):
        if not case.shuffled or case.occ.startswith("rows"):
            continue
        for ci, co in ((16, 32), (32, 32)):
            if not cg.n_ok(case.geom.K, ci, co, backward=True):
                continue
            r, tb = cg.reference(case, ci, co), cg.tables(case)
            bias = cg.signed_half_to_one(np.random.default_rng(case.seed + co), (co,))
            ref, S, n = _with_bias(case, r, bias)
            mod = _module(sp, case, ci, co, r, bias, dev)
            tensor = lambda feats: sp.SparseConvTensor(feats, T(case.idx, dev), list(case.shape), case.batch)
            mod.eval()
            with torch.no_grad():
                y = mod(tensor(T(r.x, dev)))
            assert np.array_equal(y.indices.cpu().numpy().reshape(-1, 4), tb.out_idx), case.id
            assert list(y.spatial_shape) == list(case.geom.out_shape(case.shape))
            worst.add((case.id, ci, co, "eval"), {"out": cg.ratio(y.features.cpu().numpy(), ref, S, n)})
            mod.train()
            x = T(r.x, dev).requires_grad_(True)
            y = mod(tensor(x))
            assert np.array_equal(y.indices.cpu().numpy().reshape(-1, 4), tb.out_idx), case.id
            y.features.backward(T(r.g, dev))
            q = cg.ratios(case, r, dx=x.grad.cpu().numpy(), dw=mod.weight.grad.cpu().numpy())
            q["out"] = cg.ratio(y.features.detach().cpu().numpy(), ref, S, n)
            g64 = r.g.astype(np.float64)
            q["dbias"] = cg.ratio(mod.bias.grad.cpu().numpy(), g64.sum(0), np.abs(g64).sum(0), max(tb.num_out, 1))
            worst.add((case.id, ci, co, "train"), q)
            runs += 1
    worst.report("modules", group, runs)


def test_two_subm_layers_with_different_kernels_do_not_share_a_rulebook(dev):
    from isfusion_amd import spconv as sp
    first = next(c for c in cg.CASES if c.geom.name == "subm_k333" and c.shape == (3, 4, 7) and c.occ == "full" and c.shuffled)
    second = cg.Case(cg.Geometry(True, (1, 3, 3)), first.batch, first.shape, "shared", True, first.idx)
    ci, co = 16, 32
    x = sp.SparseConvTensor(T(cg.reference(first, ci, co).x, dev), T(first.idx, dev), list(first.shape), first.batch)
    worst = Worst()
    for case in (first, second, first):
        r = cg.reference(case, ci, co)
        bias = cg.signed_half_to_one(np.random.default_rng(case.seed), (co,))
        mod = _module(sp, case, ci, co, r, bias, dev).eval()
        with torch.no_grad():
            y = mod(x.replace_feature(T(r.x, dev)))
        worst.add((case.id,), {"out": cg.ratio(y.features.cpu().numpy(), *_with_bias(case, r, bias))})
    assert len(x._rulebooks) == 2
    a, b = x._rulebooks.values()
    assert a.nbr.shape[0] + b.nbr.shape[0] == 27 + 9
    worst.report("two SubM layers", "subm_k333 + subm_k133", 3)


# ------------------------------------------------------------------------------------------------------------ refusals
REFUSED = [
    ("subm_k115", True, (1, 1, 5), (1, 1, 1), (0, 0, 0), "kernel width 5"),
    ("conv_k115", False, (1, 1, 5), (1, 1, 1), (0, 0, 2), "kernel width 5"),
    ("subm_k334", True, (3, 3, 4), (1, 1, 1), (0, 0, 0), "kernel volume 36 (max 27)"),
    ("conv_k334", False, (3, 3, 4), (1, 1, 1), (1, 1, 1), "kernel volume 36 (max 27)"),
]


@pytest.mark.parametrize("name,subm,ks,st,pd,message", REFUSED, ids=[r[0] for r in REFUSED])
def test_unsupported_kernels_are_refused_and_the_stream_stays_good(dev, name, subm, ks, st, pd, message):
    """kernel width 5 and more than 27 taps raise the library's error at the rulebook, through the function and through the
    module; a correct call straight afterwards gives the bits it gave before"""
    from isfusion_amd import _lib, spconv as sp
    case = next(c for c in cg.CASES if c.geom.name == "subm_k333" and c.shape == (3, 4, 7) and c.occ == "full" and c.shuffled)
    ci, co = 32, 32
    r = cg.reference(case, ci, co)

    def good():
        x, w = T(r.x, dev).requires_grad_(True), T(r.w, dev).requires_grad_(True)
        out = sp.SparseConvFunction.apply(x, w, _rulebook(sp, case, dev))
        return (out.detach(), *torch.autograd.grad(out, (x, w), T(r.g, dev)))

    before = good()
    Worst().add((case.id,), cg.ratios(case, r, *(t.cpu().numpy() for t in before)))
    with pytest.raises(_lib.IsfError, match=message.replace("(", r"\(").replace(")", r"\)")):
        sp.build_rulebook(T(case.idx, dev), case.batch, list(case.shape), list(ks), list(st), list(pd), subm)
    cls = sp.SubMConv3d if subm else sp.SparseConv3d
    mod = cls(16, 16, list(ks), stride=list(st), padding=list(pd)).to(dev).eval()
    with pytest.raises(_lib.IsfError, match="isf_build_rulebook failed"):
        with torch.no_grad():
            mod(sp.SparseConvTensor(T(cg.reference(case, 16, 16).x, dev), T(case.idx, dev), list(case.shape), case.batch))
    after = good()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
