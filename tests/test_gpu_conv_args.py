"""Argument checking of the exported sparse-conv entries (forward kernels and the order / table builders): the code each
bad call returns, that it returns BEFORE any kernel launch, and that the stream still computes the right bits afterwards.

The problem is the smallest one: a 16-row SubM rulebook, 27 taps, 32 -> 32 channels, nbr_stride 128 (128 -> 256 on the
one-workgroup-per-CU entry, which has no narrower shape).  A failing call gets ONE poisoned buffer for every pointer it
takes: no entry may read or write it before its checks are through, so the buffer must still hold the poison at the end.
The codes are those of IsfError's "(code N)", not the message texts."""
import ctypes
import re

import numpy as np
import pytest
import torch

from isfusion_amd import _lib

pytestmark = pytest.mark.gpu

OK, ARG, UNSUPPORTED = 0, -1, -4
POISON = 0xA5
ROWS, TAPS, STRIDE = 16, 27, 128


class Call:
    """the arguments of one call; every entry below picks what its signature takes"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def but(self, **kw):
        return Call(**{**self.__dict__, **kw})


def _conv(c):   # the 15 leading arguments most forward entries share
    return (c.xs, c.num_in, c.c_in, c.p16, c.K, c.c_out, c.nbr, c.stride, c.num_out, c.scale, c.shift, c.res, c.relu, c.out,
            c.mode)


def _parts(lib, c, dma):
    return lib.isf_sparse_conv_forward_parts(c.xs, c.num_in, c.c_in, c.p16, c.K, 0, c.c_out, c.nbr, None, c.stride, c.num_out,
                                             c.scale, c.shift, c.res, c.relu, c.out,
                                             c.mode | (_lib.CONV_MODE_DMA_PLAN if dma else 0),
                                             c.part_table_dma if dma else c.part_table, c.stream)


def _part_table(lib, c, dma):
    # `out` is the table; several rounds (flag 1) so that the 16-row launch gets one
    return lib.isf_sparse_conv_part_table(c.nbr, None, c.stride, c.K, c.num_out, c.c_in, c.c_out,
                                          c.mode | (_lib.CONV_MODE_DMA_PLAN if dma else 0), 1, c.work, 1024, c.out, 1024,
                                          c.info, c.stream)


FORWARD = {
    "f16x3": lambda lib, c: lib.isf_sparse_conv_forward_f16x3(*_conv(c), c.stream),
    "ordered": lambda lib, c: lib.isf_sparse_conv_forward_f16x3_ordered(*_conv(c), c.order, c.stream),
    "tiled": lambda lib, c: lib.isf_sparse_conv_forward_f16x3_tiled(*_conv(c), c.table, c.stream),
    "dma": lambda lib, c: lib.isf_sparse_conv_forward_dma(*_conv(c), c.order, c.stream),
    "dma_lines": lambda lib, c: lib.isf_sparse_conv_forward_dma_lines(
        c.xs, c.num_in, c.c_in, c.p16, c.K, 3, c.c_out, c.lines, c.mask, c.stride, c.num_out, c.scale, c.shift, c.res, c.relu,
        c.out, c.mode, c.stream),
    "parts": lambda lib, c: _parts(lib, c, False),
    "parts_dma": lambda lib, c: _parts(lib, c, True),
    "staged": lambda lib, c: lib.isf_sparse_conv_forward_staged(
        c.xs, c.num_in, c.c_in, c.p16, c.K, c.c_out, c.slots, c.stride, c.ulist, c.ucount, c.num_out, c.scale, c.shift, c.res,
        c.relu, c.out, 256, c.mode, c.stream),
    "cu": lambda lib, c: lib.isf_sparse_conv_forward_cu(*_conv(c)[:-1], ctypes.byref(c.plan), c.stream),
}
BUILDERS = {   # `out` is the order / table they write, `count` / `info` what they report beside it
    "tile_order": lambda lib, c: lib.isf_sparse_conv_tile_order(c.nbr, c.stride, c.K, c.num_out, c.c_in, c.c_out, c.mode,
                                                                c.work, c.out, ctypes.byref(c.count), c.stream),
    "tile_order_dma": lambda lib, c: lib.isf_sparse_conv_tile_order(c.nbr, c.stride, c.K, c.num_out, c.c_in, c.c_out,
                                                                    c.mode | _lib.CONV_MODE_DMA_PLAN, c.work, c.out,
                                                                    ctypes.byref(c.count), c.stream),
    "tile_table": lambda lib, c: lib.isf_sparse_conv_tile_table(c.nbr, c.stride, c.K, c.num_out, c.c_in, c.c_out, c.mode,
                                                                c.work, c.out, ctypes.byref(c.count), c.stream),
    "part_table": lambda lib, c: _part_table(lib, c, False),
    "part_table_dma": lambda lib, c: _part_table(lib, c, True),
}
ENTRIES = {**FORWARD, **BUILDERS}
TILE_FORWARD = ("f16x3", "ordered", "tiled", "dma", "dma_lines", "parts", "parts_dma", "staged")   # all but "cu"
ON_DMA = ("dma", "dma_lines", "parts_dma", "tile_order_dma", "part_table_dma")
SHAPE = {"cu": (128, 256)}   # the others: 32 -> 32


def _all(names, code):
    return {n: code for n in names}


# (case, what differs from the correct call, entry -> code).  An entry a case does not name has no such argument, or the
# value is a legal one there (the CU entry takes any nbr_stride >= num_out and has no mode).
BAD_CALLS = [
    ("null out", dict(out=None), _all(ENTRIES, ARG)),
    ("scale without shift", dict(scale="dummy"), _all(FORWARD, ARG)),
    ("nbr_stride 100", dict(stride=100), _all(TILE_FORWARD + tuple(BUILDERS), ARG)),
    # (the CU entry counts 28 taps as a bad rulebook, the others as a filter they were not built for)
    ("28 taps", dict(K=28), {**_all(TILE_FORWARD + tuple(BUILDERS), UNSUPPORTED), "cu": ARG}),
    ("48 -> 32", dict(c_in=48, c_out=32), _all(ENTRIES, UNSUPPORTED)),
    ("wide 128 -> 128 on the LDS-DMA kernel", dict(c_in=128, c_out=128), _all(ON_DMA, UNSUPPORTED)),
    ("narrow 64 -> 64 on the CU kernel", dict(c_in=64, c_out=64), {"cu": UNSUPPORTED}),
    ("mode 3", dict(mode=3), _all(TILE_FORWARD + tuple(BUILDERS), ARG)),
]


def _code(rc, what):
    try:
        _lib.check(rc, what)
    except _lib.IsfError as e:
        return int(re.search(r"\(code (-?\d+)\)", str(e)).group(1))
    return OK


def _dummy_call(entry, dev):
    """a correct call as far as the checks go, with one poisoned buffer behind every pointer"""
    buf = torch.full((1 << 16,), POISON, dtype=torch.uint8, device=dev)
    p = buf.data_ptr()
    c_in, c_out = SHAPE.get(entry, (32, 32))
    call = Call(xs=p, num_in=ROWS, c_in=c_in, p16=p, K=TAPS, c_out=c_out, nbr=p, stride=STRIDE, num_out=ROWS, scale=None,
                shift=None, res=None, relu=0, out=p, mode=0, order=p, table=p, part_table=p, part_table_dma=p, lines=p, mask=p,
                slots=p, ulist=p, ucount=p, plan=_lib.ConvCuPlan(), work=p, count=ctypes.c_int(-7),
                info=(ctypes.c_int * 4)(-7, -7, -7, -7), stream=_lib.stream())
    return call, buf


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_zero_rows_is_ok_and_touches_nothing(dev, entry):
    call, buf = _dummy_call(entry, dev)
    assert _code(ENTRIES[entry](_lib.load(), call.but(num_out=0)), entry) == OK
    if entry in ("tile_order", "tile_order_dma", "tile_table"):
        assert call.count.value == 0
    if entry in ("part_table", "part_table_dma"):
        assert list(call.info) == [0, 0, 0, 0]
    torch.cuda.synchronize()
    assert bool((buf == POISON).all())


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_bad_calls_return_their_code_before_any_launch(dev, entry):
    call, buf = _dummy_call(entry, dev)
    lib = _lib.load()
    seen = 0
    for case, diff, codes in BAD_CALLS:
        if entry not in codes:
            continue
        diff = {k: (buf.data_ptr() if v == "dummy" else v) for k, v in diff.items()}
        got = _code(ENTRIES[entry](lib, call.but(**diff)), entry)
        print(f"{entry}: {case}: code {got}")
        assert got == codes[entry], (entry, case)
        seen += 1
    assert seen >= 3
    torch.cuda.synchronize()
    assert bool((buf == POISON).all())


_cases = {}


def _real_case(dev, c_in, c_out):
    """the 16-row problem with real buffers, and its result on isf_sparse_conv_forward_f16x3 (computed once per shape)"""
    if (c_in, c_out) not in _cases:
        from isfusion_amd import spconv as sp
        rng = np.random.default_rng(c_in + c_out)
        shape = [4, 4, 4]
        lin = np.sort(rng.choice(64, ROWS, replace=False))
        idx = np.stack([lin * 0, lin // 16, (lin // 4) % 4, lin % 4], 1).astype(np.int32)
        rb = sp.build_rulebook(torch.from_numpy(idx).to(dev), 1, shape, [3, 3, 3], [1, 1, 1], [1, 1, 1], True)
        assert rb.num_out == ROWS and rb.stride == STRIDE
        x = torch.from_numpy(rng.normal(0, 1, (ROWS, c_in)).astype(np.float32)).to(dev)
        w = torch.from_numpy(rng.normal(0, (1.0 / (6 * c_in)) ** 0.5, (3, 3, 3, c_in, c_out)).astype(np.float32)).to(dev)
        scale = torch.from_numpy(rng.random(c_out, dtype=np.float32) + 0.5).to(dev)
        shift = torch.from_numpy(rng.normal(0, 0.2, c_out).astype(np.float32)).to(dev)
        res = torch.from_numpy(rng.normal(0, 1, (ROWS, c_out)).astype(np.float32)).to(dev)
        p16 = sp.pack_filters_f16x3(w)
        ref = sp.sparse_conv_forward_f16x3(x, p16, TAPS, c_in, c_out, rb, scale, shift, res, relu=True)
        assert ref.abs().max() > 0.5
        _cases[(c_in, c_out)] = (rb, sp.to_split(x), p16, scale, shift, sp.to_split(res), ref)
    return _cases[(c_in, c_out)]


@pytest.mark.parametrize("entry", list(FORWARD))
def test_a_correct_call_after_an_error_computes_the_reference_bits(dev, entry):
    from isfusion_amd import spconv as sp
    lib = _lib.load()
    c_in, c_out = SHAPE.get(entry, (32, 32))
    rb, xs, p16, scale, shift, rs, ref = _real_case(dev, c_in, c_out)
    ys = torch.full((ROWS * c_out * 4,), POISON, dtype=torch.uint8, device=dev)
    call = Call(xs=xs.data_ptr(), num_in=ROWS, c_in=c_in, p16=p16.data_ptr(), K=TAPS, c_out=c_out, nbr=rb.nbr.data_ptr(),
                stride=rb.stride, num_out=ROWS, scale=scale.data_ptr(), shift=shift.data_ptr(), res=rs.data_ptr(), relu=1,
                out=ys.data_ptr(), mode=0, order=None, stream=_lib.stream())
    keep = []   # the tables an entry reads, alive until the result is back
    if entry == "tiled":
        keep.append(sp.tile_table(rb, c_in, c_out))
        call.table = keep[0].data_ptr()
    if entry in ("parts", "parts_dma"):
        keep.append(sp.part_table(rb, c_in, c_out, dma=entry == "parts_dma", several_rounds=True))
        call.part_table = call.part_table_dma = keep[0].table.data_ptr()
    if entry == "dma_lines":
        lines, mask, flag = keep_lines = sp.rulebook_lines(rb, 3)
        assert int(flag.item()) == 0
        keep.append(keep_lines)
        call.lines, call.mask = lines.data_ptr(), mask.data_ptr()
    if entry == "staged":
        keep.append(sp.stage_tables(rb))
        call.slots, call.ulist, call.ucount = (t.data_ptr() for t in keep[0])
    if entry == "cu":
        keep.append(sp.cu_plan(rb))
        call.plan = keep[0][0]
    for diff, code in ((dict(out=None), ARG), (dict(c_in=48, c_out=32), UNSUPPORTED)):
        assert _code(ENTRIES[entry](lib, call.but(**diff)), entry) == code
    assert _code(ENTRIES[entry](lib, call), entry) == OK
    got = sp.from_split(ys, (ROWS, c_out))
    assert torch.equal(got, ref), (entry, (got - ref).abs().max().item())
