"""Cross-rank float sums that do not depend on the collective: the deterministic mode across ranks.

A float all-reduce rounds after every add, so its bits depend on the library's algorithm, its channel and protocol choice
and the layout of the ranks.  Here a rank turns its contribution into 64-bit fixed point (csrc/isf_fixed.h, with N = the
world size), the collective adds INTEGERS -- the same in every order -- and the sum is converted back once: the result is a
function of the multiset of the ranks' contributions only.  RCCL on eight devices, gloo on one, the ranks in any order:
the same bits.

all_reduce_sum_             one short vector (the [2C] statistics of naiveSyncBN): all_gather + isf_fixed_sum_rows when
                            `exact`, dist.all_reduce(SUM) -- the call the sites made before -- otherwise.
exact_all_reduce_gradients  every gradient of a model after a backward pass that ran without DDP's own reduction
                            (`with ddp.no_sync():`): absmax launch, int32 MAX all-reduce of the bounds, pack launch, int64
                            SUM all-reduce of one flat buffer, finish launch.  No host sync.

A tensor with a non-finite contribution on any rank comes back all-NaN on every rank.  There is no fallback: CPU, non-fp32
or non-contiguous tensors raise IsfError."""
import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from ._lib import IsfError

CHUNK = _lib.OPTIM_CHUNK
MAX_WORLD = 1024             # log2_world <= 10: |q| <= 2^52 still resolves an fp32 contribution to 2^-28 of the bound


def ceil_log2(n):
    return max(int(n) - 1, 0).bit_length()


def _check(t, what):
    if not isinstance(t, torch.Tensor):
        raise IsfError(f"{what}: expected a tensor, got {type(t).__name__}")
    if t.is_sparse or t.layout != torch.strided:
        raise IsfError(f"{what}: sparse tensors are not supported by the exact reductions")
    if not t.is_cuda:
        raise IsfError(f"{what}: the exact reductions run on the GPU only (HIP kernels); got a CPU tensor. "
                       "There is deliberately no CPU fallback.")
    if t.dtype != torch.float32:
        raise IsfError(f"{what}: the exact reductions take float32 tensors, got {t.dtype}")
    if not t.is_contiguous():
        raise IsfError(f"{what}: the exact reductions take contiguous tensors")


# ------------------------------------------------------------------------------------------------ one short vector
def sum_rows(rows, divisor=1.0, out=None):
    """out [n] = the exact column sums of rows [W, n] (W <= 64) / divisor, rounded once (isf_fixed_sum_rows): independent
    of the order of the rows; a column with a non-finite value is NaN."""
    _check(rows, "rows")
    if rows.dim() != 2 or not 1 <= rows.shape[0] <= _lib.FIXED_MAX_ROWS:
        raise IsfError(f"rows: expected [W, n] with 1 <= W <= {_lib.FIXED_MAX_ROWS}, got {tuple(rows.shape)}")
    w, n = rows.shape
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=rows.device)
    else:
        _check(out, "out")
        if out.numel() != n or out.device != rows.device:
            raise IsfError(f"out: {out.numel()} elements on {out.device} for rows {tuple(rows.shape)} on {rows.device}")
    _lib.check(_lib.load().isf_fixed_sum_rows(_lib.ptr(rows), w, n, float(divisor), _lib.ptr(out), _lib.stream()),
               "isf_fixed_sum_rows")
    return out


def all_reduce_sum_(t, exact, group=None):
    """In-place sum of `t` over the ranks of `group`.  exact false, or one rank: dist.all_reduce(t, SUM).  exact true: every
    rank gathers the W contributions ([W, n], one collective) and adds them exactly (one launch) -- the reference's own
    all_gather + sum (mmdet3d/ops/norm.py:12-19), made independent of the order.  -> t"""
    if not exact or dist.get_world_size(group) == 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        return t
    _check(t, "all_reduce_sum_")
    world = dist.get_world_size(group)
    if world > _lib.FIXED_MAX_ROWS:
        raise IsfError(f"all_reduce_sum_: the exact sum of a gathered vector takes up to {_lib.FIXED_MAX_ROWS} ranks, "
                       f"got {world}")
    flat = t.view(-1)
    rows = torch.empty(world, flat.numel(), dtype=torch.float32, device=t.device)
    dist.all_gather(list(rows.unbind(0)), flat, group=group)
    sum_rows(rows, 1.0, out=flat)
    return t


# ------------------------------------------------------------------------------------------------ many tensors
class TensorTable:
    """The device tables of one list of fp32 tensors for the isf_fixed_*_tensors entries: int64 [T, 3] = address, numel,
    offset in the flat fixed-point buffer, then int32 [C, 2] = tensor, chunk; the uint32 bounds [T] (handed to the
    collective as int32: a pattern of |x| has no sign bit) and the int64 buffer `q` [sum of numel].  Built once per set of
    addresses; the upload goes through pinned memory and waits for nothing."""

    def __init__(self, tensors):
        for i, t in enumerate(tensors):
            _check(t, f"tensor {i}")
            if t.device != tensors[0].device:
                raise IsfError(f"tensor {i}: tensors on {tensors[0].device} and {t.device}; one reduction runs on one device")
        self.device = dev = tensors[0].device
        numel = np.array([t.numel() for t in tensors], np.int64)
        self.num_tensors = n = len(tensors)
        self.total = int(numel.sum())
        counts = (numel + CHUNK - 1) // CHUNK
        self.num_chunks = c = int(counts.sum())
        host = np.zeros(3 * n + c, np.int64)
        tab = host[:3 * n].reshape(n, 3)
        tab[:, 0] = [t.data_ptr() for t in tensors]
        tab[:, 1] = numel
        tab[:, 2] = np.cumsum(numel) - numel
        ch = host[3 * n:].view(np.int32).reshape(c, 2)
        ch[:, 0] = np.repeat(np.arange(n, dtype=np.int32), counts)
        ch[:, 1] = np.arange(c, dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)
        pinned = torch.from_numpy(host).pin_memory()
        self.table = torch.empty(host.size, dtype=torch.int64, device=dev)
        self.table.copy_(pinned, non_blocking=True)
        self._pinned = pinned                              # alive until the copy has run: as long as the table
        self.bits = torch.zeros(n, dtype=torch.int32, device=dev)
        self.q = torch.empty(max(self.total, 1), dtype=torch.int64, device=dev)

    def _args(self):
        base = self.table.data_ptr()
        return base, base + 8 * 3 * self.num_tensors, self.num_chunks

    def absmax(self):
        """bits[t] = largest bit pattern of |x| in tensor t (this rank)"""
        tab, chk, c = self._args()
        _lib.check(_lib.load().isf_fixed_absmax_tensors(tab, chk, c, self.num_tensors, self.bits.data_ptr(), _lib.stream()),
                   "isf_fixed_absmax_tensors")

    def pack(self, log2_world, q=None):
        """q = the tensors in fixed point under the bounds in `bits` (the maximum over the ranks by now)"""
        tab, chk, c = self._args()
        q = self.q if q is None else q
        _lib.check(_lib.load().isf_fixed_pack_tensors(tab, chk, c, self.bits.data_ptr(), int(log2_world), q.data_ptr(),
                                                      _lib.stream()), "isf_fixed_pack_tensors")
        return q

    def finish(self, log2_world, divisor, q=None):
        """the tensors = q (the sum over the ranks by now) / divisor, NaN where the bound is not finite"""
        tab, chk, c = self._args()
        q = self.q if q is None else q
        _lib.check(_lib.load().isf_fixed_finish_tensors(tab, chk, c, self.bits.data_ptr(), int(log2_world), q.data_ptr(),
                                                        float(divisor), _lib.stream()), "isf_fixed_finish_tensors")


_TABLES = {}


def _named(params):
    if isinstance(params, torch.nn.Module):
        return [(n, p) for n, p in params.named_parameters() if p.requires_grad]
    out = []
    for i, item in enumerate(params):
        name, p = item if isinstance(item, tuple) else (f"parameter {i}", item)
        out.append((name, p))
    return out


@torch.no_grad()
def exact_all_reduce_gradients(params, group=None, average=True):
    """Every `.grad` of `params` (parameters, (name, parameter) pairs, or a module: its parameters that require a gradient)
    becomes the exact sum of the ranks' gradients -- divided by the world size when `average`, DDP's convention -- rounded
    once to fp32: the same bits on every rank, under every order of the ranks and every backend.  Call it after a backward
    pass whose gradients are still local (`with ddp.no_sync():`).  Five steps, two of them collectives, no host sync; the
    tables and the int64 buffer are cached per set of gradient addresses.  One rank: nothing to do."""
    world = dist.get_world_size(group)
    if world == 1:
        return
    if world > MAX_WORLD:
        raise IsfError(f"exact_all_reduce_gradients: up to {MAX_WORLD} ranks, got {world}")
    grads = []
    for name, p in _named(params):
        if p.grad is None:
            raise IsfError(f"exact_all_reduce_gradients: {name} {tuple(p.shape)} has no gradient; every rank must "
                           "contribute every listed tensor (freeze unused parameters instead of listing them)")
        grads.append(p.grad)
    if not grads:
        return
    try:
        key = tuple((g.data_ptr(), g.numel()) for g in grads)
    except RuntimeError:                             # no strided storage (sparse): TensorTable says why
        key = None
    table = _TABLES.get(key)
    if table is None:
        if len(_TABLES) >= 8:
            _TABLES.clear()
        table = TensorTable(grads)
        if key is not None:
            _TABLES[key] = table
    log2_world = ceil_log2(world)
    table.absmax()
    dist.all_reduce(table.bits, op=dist.ReduceOp.MAX, group=group)
    table.pack(log2_world)
    dist.all_reduce(table.q, op=dist.ReduceOp.SUM, group=group)
    table.finish(log2_world, world if average else 1)
