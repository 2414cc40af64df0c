"""The geometry sweep on the CPU: the float64 dense-conv3d reference of tests/conv_geometry_common.py against the oracle
restatement of the reference's sparse convolution (get_indice_pairs / indice_conv / indice_conv_backward) on every case,
mutation checks of the comparator, and the case table's own conditions.  No GPU."""
import numpy as np
import pytest

import conv_geometry_common as cg

C_IN, C_OUT = 5, 16


def _oracle_case(oracle, case):
    """the oracle's active set and pair lists in OUR output-row order -> (pairs int32 [K, 2, n], num [K])"""
    g = case.geom
    out_idx, pairs, num = oracle.get_indice_pairs(case.idx, case.batch, case.shape, g.ks, g.st, g.pd, subm=g.subm)
    tb = cg.tables(case)
    ours = {tuple(int(v) for v in c): o for o, c in enumerate(tb.out_idx)}
    theirs = [tuple(int(v) for v in c) for c in out_idx]
    assert len(set(theirs)) == len(theirs) and set(theirs) == set(ours), case.id
    if g.subm:
        assert theirs == [tuple(int(v) for v in c) for c in case.idx], case.id
    remap = np.array([ours[c] for c in theirs], np.int32)
    pairs = pairs.copy()
    for k in range(g.K):
        pairs[k, 1, :num[k]] = remap[pairs[k, 1, :num[k]]]
    return pairs, num.copy()


def _run(oracle, case, r, pairs, num, w=None):
    tb = cg.tables(case)
    w = r.w if w is None else w
    out = oracle.indice_conv(r.x, w, pairs, num, tb.num_out)
    dx, dw = oracle.indice_conv_backward(r.x, w, r.g, pairs, num)
    return out, dx, dw


@pytest.mark.parametrize("group", cg.GROUPS)
def test_reference_matches_the_oracle(oracle_mod, group):
    worst = {}
    for case in cg.cases_of(group):
        tb = cg.tables(case)
        r = cg.reference(case, C_IN, C_OUT)
        assert np.array_equal(r.out_idx, tb.out_idx), case.id            # the mask conv's active set == brute force
        pairs, num = _oracle_case(oracle_mod, case)
        for k in range(case.geom.K):
            got = set(zip(pairs[k, 0, :num[k]].tolist(), pairs[k, 1, :num[k]].tolist()))
            assert got == set(zip(tb.pairs[k][0].tolist(), tb.pairs[k][1].tolist())), (case.id, k)
        q = cg.ratios(case, r, *_run(oracle_mod, case, r, pairs, num))
        for name, v in q.items():
            assert v <= 1.0, (case.id, name, v)
            worst[name] = max(worst.get(name, 0.0), v)
    print(f"{group}: worst err / bound {worst}")


def _busiest(num):
    return int(np.argmax(num))


@pytest.mark.parametrize("group", cg.GROUPS)
def test_mutations_fail_the_comparator(oracle_mod, group):
    """each subtly wrong kernel must exceed the bound on every case where it changes anything"""
    seen = dict(dropped=0, swapped=0, shifted=0, unwritten=0, unreached=0)
    for case in cg.cases_of(group):
        tb = cg.tables(case)
        if tb.num_out == 0:
            continue
        r = cg.reference(case, C_IN, C_OUT)
        pairs, num = _oracle_case(oracle_mod, case)
        kb = _busiest(num)
        assert num[kb] >= 1
        good = _run(oracle_mod, case, r, pairs, num)
        # one pair dropped from the busiest tap: out, dX and dW each miss one product (row)
        p2, n2 = pairs.copy(), num.copy()
        n2[kb] -= 1
        p2[kb, :, n2[kb]] = -1
        q = cg.ratios(case, r, *_run(oracle_mod, case, r, p2, n2))
        assert min(q.values()) > 1.0, (case.id, "dropped", q)
        seen["dropped"] += 1
        # two taps' weight slices swapped
        if case.geom.K >= 2:
            w2 = r.w.copy().reshape(case.geom.K, C_IN, C_OUT)
            ko = (kb + 1) % case.geom.K
            w2[[kb, ko]] = w2[[ko, kb]]
            q = cg.ratios(case, r, out=_run(oracle_mod, case, r, pairs, num, w2.reshape(r.w.shape))[0])
            assert q["out"] > 1.0, (case.id, "swapped", q)
            seen["swapped"] += 1
        # a tap's neighbours shifted by one row
        if case.n >= 2:
            p2 = pairs.copy()
            p2[kb, 0, :num[kb]] = (p2[kb, 0, :num[kb]] + 1) % case.n
            q = cg.ratios(case, r, *_run(oracle_mod, case, r, p2, num))
            assert q["out"] > 1.0 and q["dw"] > 1.0, (case.id, "shifted", q)
            seen["shifted"] += 1
        # one dW tap slice left unwritten (zeros, or what the buffer held)
        for stale in (0.0, 1.0):
            dw2 = good[2].copy().reshape(case.geom.K, C_IN, C_OUT)
            dw2[kb] = stale
            assert cg.ratios(case, r, dw=dw2.reshape(r.w.shape))["dw"] > 1.0, (case.id, "unwritten", stale)
        seen["unwritten"] += 1
        # one unreached dX row non-zero
        unreached = np.nonzero((tb.nbr_t < 0).all(0))[0]
        if unreached.size:
            assert not r.s_dx[unreached].any() and not good[1][unreached].any(), case.id
            dx2 = good[1].copy()
            dx2[unreached[-1], C_IN - 1] = 1e-30
            assert cg.ratios(case, r, dx=dx2)["dx"] == np.inf, (case.id, "unreached")
            seen["unreached"] += 1
    print(f"{group}: mutations applied {seen}")
    assert seen["dropped"] and seen["unwritten"]


def test_a_dropped_pair_is_far_above_the_bound_and_unused_taps_are_exact_zeros(oracle_mod):
    """the margin on one case: a dropped pair exceeds the bound 100-fold, and a one-cell-thick grid under a 3-wide kernel
    has taps no pair uses, whose dW reference and S are exactly 0"""
    case = next(c for c in cg.CASES if c.geom.name == "subm_k333" and c.shape == (4, 5, 1) and c.occ == "full" and not c.shuffled)
    tb = cg.tables(case)
    assert (tb.counts == 0).sum() == 18               # kx = 0 and kx = 2 of every line
    r = cg.reference(case, C_IN, C_OUT)
    unused = tb.counts == 0
    assert not r.s_dw.reshape(case.geom.K, -1)[unused].any() and not r.dw.reshape(case.geom.K, -1)[unused].any()
    pairs, num = _oracle_case(oracle_mod, case)
    kb = _busiest(num)
    num[kb] -= 1
    q = cg.ratios(case, r, *_run(oracle_mod, case, r, pairs, num))
    assert min(q.values()) > 100.0, q


def test_the_static_drop_rule_drops_what_it_predicts():
    all_combos = cg.combos()
    dropped = [(g, b, s, o) for g, b, s, o in all_combos if not g.fits(s)]
    assert len(all_combos) == 525 and len(dropped) == 72
    for g, b, s, o in all_combos:               # the rule is the output shape's: empty <=> dropped; SubM never
        assert g.fits(s) == all(v > 0 for v in g.out_shape(s)), (g.name, s)
    assert not any(g.subm for g, _, _, _ in dropped)
    kept = {(c.geom.name, c.batch, c.shape, c.occ) for c in cg.CASES if not c.occ.startswith("rows")}
    assert len(kept) == 525 - 72


def test_every_case_is_inside_the_comparators_range():
    assert 4 * cg.MAX_N * cg.c_of(cg.MAX_N) < 1 <= 4 * (cg.MAX_N + 1) * cg.c_of(cg.MAX_N + 1)
    shapes = {s for f in cg.FAMILIES.values() for s in f}
    for case in cg.CASES:
        assert 1 <= case.n <= cg.MAX_ROWS, case.id
        assert len({tuple(c) for c in case.idx.tolist()}) == case.n
        ranked = np.lexsort(case.idx.T[::-1])
        assert case.shuffled != np.array_equal(ranked, np.arange(case.n)), case.id
        counts = cg.tables(case).counts
        assert counts.max(initial=0) <= cg.MAX_N and 4 * counts.max(initial=0) * cg.c_of(counts.max(initial=0)) < 1
        for family in cg.FAMILIES:
            for c_in, c_out in cg.family_shapes(family, case):
                n = case.geom.K * c_in
                assert 4 * n * cg.c_of(n) < 1
        for c_in, c_out in cg.BACKWARD_SPLIT + cg.BACKWARD_FP32:
            if cg.n_ok(case.geom.K, c_in, c_out, backward=True):
                n = case.geom.K * max(c_in, c_out)
                assert 4 * n * cg.c_of(n) < 1
    assert cg.n_ok(18, 64, 64) and not cg.n_ok(25, 64, 64) and cg.n_ok(9, 128, 32) and not cg.n_ok(18, 128, 32)
    assert all(cg.n_ok(27, 32, c) for c in (32, 64, 128, 256)) and shapes


# the tap counts each family can take inside the comparator's range (K Cin <= 1179 at its narrowest shape; the
# line-compressed table: x-lines of three taps, or single taps, nine lines at the most)
FAMILY_K = {
    "fp32_mfma": cg.K_REQUIRED, "generic": cg.K_REQUIRED, "tile": cg.K_REQUIRED, "dma": cg.K_REQUIRED, "staged": cg.K_REQUIRED,
    "best": cg.K_REQUIRED, "cu": (1, 3, 6, 8, 9), "dma_lines3": (3, 9, 27), "dma_lines1": (1, 3, 6, 8, 9),
}


def test_every_required_tap_count_is_present_for_every_family():
    assert set(FAMILY_K) == set(cg.FAMILIES)
    assert {g.K for g in cg.GEOMETRIES} >= set(cg.K_REQUIRED) | {2}
    for family, want in FAMILY_K.items():
        for shuffled in (False, True):
            have = {c.geom.K for c in cg.CASES if c.shuffled == shuffled and c.n > 16 and cg.family_shapes(family, c)}
            if family == "dma_lines3" and shuffled:
                assert not have
                continue
            assert have & set(cg.K_REQUIRED) == set(want), (family, shuffled, sorted(have))
    for c_in, c_out in cg.BACKWARD_SPLIT + cg.BACKWARD_FP32:
        have = {c.geom.K for c in cg.CASES if cg.n_ok(c.geom.K, c_in, c_out, backward=True)}
        assert have >= {1, 2, 3, 6, 8, 9}, (c_in, c_out)
    # row counts on either side of the 16-row group, the 64-row tile, the 128-row table pad and the 256-thread block
    for name in ("subm_k333", "conv_k333_s222_p111"):
        assert {c.n for c in cg.CASES if c.geom.name == name and c.occ.startswith("rows")} == set(cg.ROW_COUNTS)
