"""GPU tests of the cross-rank exact sums (isfusion_amd.collectives; isf_fixed_absmax_tensors / _pack_tensors /
_finish_tensors / isf_fixed_sum_rows of include/isf_hip.h).  The kernels are compared BIT FOR BIT with the big-integer model
of tests/collectives_common.py -- there is no tolerance -- on views at odd 4-byte offsets, under two orders of the integer
sum of simulated ranks, under permutations of gathered rows; the last test runs three gloo ranks on one device
(tests/collectives_check.py): the same digest of a three-step training run for two ways of dealing the data to the ranks."""
import os
import subprocess

import numpy as np
import pytest
import torch

import collectives_common as CM

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 7.0


def _place(arrays):
    """the arrays as views of ONE flat device buffer, at offsets whose residue mod 4 elements keeps changing (DDP's bucket
    views sit at any 4-byte offset); the gaps hold a sentinel.  -> (buffer, views, [(offset, numel)])"""
    spans, off = [], 1
    for i, a in enumerate(arrays):
        spans.append((off, a.size))
        off += a.size + 1 + i % 3
    host = np.full(off, SENTINEL, np.float32)
    for (o, n), a in zip(spans, arrays):
        host[o:o + n] = a
    buf = torch.from_numpy(host).to(DEV)
    return buf, [buf[o:o + n] for o, n in spans], spans


def _gaps_untouched(buf, spans):
    host = buf.cpu().numpy()
    keep = np.ones(host.size, bool)
    for o, n in spans:
        keep[o:o + n] = False
    return bool((host[keep] == SENTINEL).all())


@pytest.fixture(scope="module")
def case_a():
    """every count x every magnitude, as one tensor list; the model's bound, packed integers and finish per tensor"""
    rs = np.random.RandomState(21)
    arrays = [CM.tensor_of(kind, n, rs) for n in CM.COUNTS for kind in CM.KINDS]
    kinds = [kind for _ in CM.COUNTS for kind in CM.KINDS]
    log2_world, divisor = 3, 8.0
    model = []
    for a in arrays:
        bits = CM.bound_bits(a)
        e = CM.exponent(bits, log2_world)
        q = CM.pack(a, e)
        model.append((bits, q, CM.finish(q, e, divisor)))
    return arrays, kinds, log2_world, divisor, model


# ------------------------------------------------------------------------------------------------ (a) the three passes
def test_absmax_pack_finish_equal_the_model_on_views_at_odd_offsets(case_a):
    from isfusion_amd import collectives
    arrays, kinds, log2_world, divisor, model = case_a
    buf, views, spans = _place(arrays)
    assert {v.data_ptr() % 16 for v in views} == {0, 4, 8, 12}                       # every residue of the float4 path
    table = collectives.TensorTable(views)
    assert table.num_chunks == len(arrays) + sum(n > collectives.CHUNK for n in CM.COUNTS) * len(CM.KINDS)
    table.bits.fill_(-1)                                                              # the entry zeroes the bounds itself
    table.absmax()
    bits = table.bits.cpu().numpy().view(np.uint32)
    assert [int(b) for b in bits] == [m[0] for m in model]
    for b, kind in zip(bits, kinds):
        assert (b >= CM.INF_BITS) == (kind in ("nan", "inf")) and (b == 0) == (kind == "zero")
    assert CM.same_bits(torch.cat(views).cpu().numpy(), np.concatenate(arrays))      # absmax reads only
    table.q.fill_(-12345)
    q = table.pack(log2_world).cpu().numpy()
    assert q.size == sum(a.size for a in arrays)
    assert q.tolist() == [v for m in model for v in m[1]]
    assert _gaps_untouched(buf, spans)
    table.finish(log2_world, divisor)
    for v, kind, (_, _, want), a in zip(views, kinds, model, arrays):
        got = v.cpu().numpy()
        if kind in ("nan", "inf"):
            assert np.isnan(got).all(), kind                                           # loud, and confined to the tensor
        else:
            assert CM.same_bits(got, want), (kind, a.size)
            if kind != "zero":
                bound = float(np.abs(a).max())                                         # (the model is no tautology: x / 8,
                assert np.allclose(got * np.float32(divisor), a, rtol=1e-6, atol=bound * 2.0 ** -40)   # to the resolution)
    assert _gaps_untouched(buf, spans)


# ------------------------------------------------------------------------------------------------ (b) simulated ranks
@pytest.mark.parametrize("world", [3, 8])
def test_simulated_ranks_sum_to_the_model_in_every_order(world):
    from isfusion_amd import collectives
    shapes = [(n, kind) for n in (3, 513, 4097) for kind in ("mixed", "tiny", "unit")]
    contribs = [[CM.tensor_of(kind, n, np.random.RandomState(100 * world + 10 * r + i)) for i, (n, kind) in enumerate(shapes)]
                for r in range(world)]
    log2_world = CM.ceil_log2(world)
    placed = [_place(c) for c in contribs]
    tables = [collectives.TensorTable(views) for _, views, _ in placed]
    for t in tables:
        t.absmax()
    bound = torch.stack([t.bits for t in tables]).max(dim=0).values                   # the MAX all-reduce of the bounds
    packed = []
    for t in tables:
        t.bits.copy_(bound)
        packed.append(t.pack(log2_world).clone())
    forward, backward = list(range(world)), list(range(world))[::-1]
    sums = []
    for order in (forward, backward):                                                 # the SUM all-reduce, two orders
        s = torch.zeros_like(packed[0])
        for r in order:
            s += packed[r]
        sums.append(s)
    outs = []
    for s in sums:
        tables[0].finish(log2_world, float(world), q=s)
        outs.append([v.clone() for v in placed[0][1]])
    assert torch.equal(sums[0], sums[1])
    for i in range(len(shapes)):
        want = CM.reduce_tensor([contribs[r][i] for r in range(world)], float(world))
        assert int(bound[i]) == want[0]
        assert torch.equal(outs[0][i], outs[1][i]) and CM.same_bits(outs[0][i].cpu().numpy(), want[3]), shapes[i]
    assert _gaps_untouched(placed[0][0], placed[0][2])
    # the float sum of the same contributions shows the order (why the integers are there)
    rows = np.stack([np.concatenate(c) for c in contribs])
    assert not CM.same_bits(CM.sequential_sum(rows, forward), CM.sequential_sum(rows, backward))


# ------------------------------------------------------------------------------------------------ (c) gathered rows
@pytest.mark.parametrize("n", [2, 128, 1024])
@pytest.mark.parametrize("world", [1, 2, 3, 8, 64])
def test_sum_rows_is_exact_order_free_and_confines_a_poisoned_column(world, n):
    from isfusion_amd import collectives
    rs = np.random.RandomState(1000 * world + n)
    rows = CM.mixed(rs, (world, n))
    rows[:, 0] = 0.0                                                                  # an all-zero column
    want = CM.sum_rows(rows, float(world))
    dev_rows = torch.from_numpy(rows).to(DEV)
    got = collectives.sum_rows(dev_rows, float(world))
    assert CM.same_bits(got.cpu().numpy(), want) and want[0] == 0.0
    for _ in range(2):
        perm = torch.from_numpy(rs.permutation(world)).to(DEV)
        assert torch.equal(collectives.sum_rows(dev_rows[perm].contiguous(), float(world)), got)
    bad = rows.copy()
    bad[world // 2, 1] = np.nan
    bad[0, n - 1] = np.inf
    out = torch.full((n + 2,), SENTINEL, device=DEV)
    collectives.sum_rows(torch.from_numpy(bad).to(DEV), float(world), out=out[1:n + 1])
    host = out.cpu().numpy()
    assert host[0] == SENTINEL and host[n + 1] == SENTINEL
    poisoned = np.zeros(n, bool)
    poisoned[[1, n - 1]] = True
    assert np.isnan(host[1:n + 1][poisoned]).all()
    assert CM.same_bits(host[1:n + 1][~poisoned], want[~poisoned])
    assert CM.same_bits(host[1:n + 1], CM.sum_rows(bad, float(world)))


# ------------------------------------------------------------------------------------------------ (d) three gloo ranks
def test_three_ranks_train_to_the_same_bits_however_the_data_are_dealt():
    """tests/collectives_check.py under torch.distributed.run: with the mode on the digest of parameters, BN buffers and
    reduced gradients after three steps is the same for the data orders 0,1,2 and 2,0,1, and the gradients sit as close
    to the float64 restatement as the float all-reduce's do (the project's camera convention: err <= 2 * err of the same
    launch with the mode off + 1e-6 * max|ref|).  What the mode-off digests do under the permutation is printed only."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    from isfusion_amd import launch
    cmd = launch.launch_command(os.path.join(root, "tests", "collectives_check.py"), [], 3, launch.free_port())
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l.split() for l in p.stdout.decode().splitlines() if l.startswith("COLLECTIVES_")]
    print("\n".join(" ".join(l) for l in lines), file=sys.stderr)
    digest = {(l[1], l[2]): l[3] for l in lines if l[0] == "COLLECTIVES_DIGEST"}
    agree = {(l[1], l[2]): l[5] for l in lines if l[0] == "COLLECTIVES_DIGEST"}
    assert set(digest) == {(m, o) for m in ("on", "off") for o in ("0,1,2", "2,0,1")}, lines
    assert digest["on", "0,1,2"] == digest["on", "2,0,1"], digest
    assert agree["on", "0,1,2"] == agree["on", "2,0,1"] == "1", agree
    err = {l[1]: (float(l[2]), float(l[4])) for l in lines if l[0] == "COLLECTIVES_GRAD_ERR"}
    assert err["on"][1] > 0 and err["on"][0] <= 2 * err["off"][0] + 1e-6 * err["on"][1], err
    assert [l for l in lines if l[0] == "COLLECTIVES_REFUSALS"] == [["COLLECTIVES_REFUSALS", "1"]], lines
